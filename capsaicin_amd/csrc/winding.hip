// winding.hip — generalised winding numbers (Jacobson et al. 2013) over the scene's binary tree, gfx950: the first-order dipole table of
// cap_winding_build (Barill et al. 2018) and the walk of cap_winding_numbers.  include/capsaicin_hip.h ("winding numbers") has the
// definitions; DESIGN.md "Winding numbers" the reasons.
//
// The table follows the TRAVERSAL links of the tree (q3.z, q3.w of a node: a subtree of at most kLeafMax triangles is one leaf, a range
// of the leaf order), because those are what the walk follows.  Build (one stream, no host round trip):
//   k_wn_triangles  per leaf-order position: n_t, a_t and a_t c_t of the triangle's ORIGINAL vertices in binary64, zeros for a degenerate one
//   k_wn_links      parent links (node << 1) | slot of the inner traversal children, as refit.hip's k_refit_links derives the binary ones
//   k_wn_climb      one thread per (node, slot) whose child is a leaf: the leaf's sums in leaf order, then up the links; the first thread
//                   to reach a node leaves, the second adds slot 0 + slot 1 and carries the sum to the parent's slot
//   k_wn_records    per (node, slot): p~, r, N and the child code from the slot's sums and the child's stored box
// Every sum has one fixed order, so the bytes of the table do not depend on which thread arrives first.  Nodes below a traversal leaf
// are never walked; their records are filled by the same rule (both their children are leaves) and nothing climbs from them.
#include "cap_kernels.h"
#include "cap_leaf.h"
#include "cap_query_walk.h"  // with_stack_class, launch_points

namespace cap
{
namespace
{
constexpr uint32_t kNoParent = 0xffffffffu;

// dot of the contract: no fused multiply-add (the build has -ffp-contract=off)
__device__ __forceinline__ float  dot_c(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
__device__ __forceinline__ double ddot(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

__device__ __forceinline__ double load_agent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- the table ----
__global__ __launch_bounds__(kBlock) void k_wn_triangles(WindingBuildArgs a)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.tri_count) return;
    const uint32_t g  = a.leaf_tri[i];
    const uint4    id = a.tri_ids[g];
    const uint4    mo = a.mesh_offsets[id.x];
    const uint32_t io = mo.y + 3u * id.y;
    double         p[3][3];
    bool           finite = true;
    for (int k = 0; k < 3; ++k)
    {
        const uint32_t v = mo.x + a.indices[io + k];
        for (int j = 0; j < 3; ++j)
        {
            const float x = a.positions[3 * (size_t)v + j];
            finite        = finite && fabsf(x) < __builtin_inff();  // (a NaN fails the comparison)
            p[k][j]       = (double)x;
        }
    }
    const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
    const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
    const double nx = 0.5 * (e1y * e2z - e1z * e2y), ny = 0.5 * (e1z * e2x - e1x * e2z), nz = 0.5 * (e1x * e2y - e1y * e2x);
    double* const s = a.tri_sums + 7 * (size_t)i;
    if (!finite || (nx == 0.0 && ny == 0.0 && nz == 0.0))
    {
        for (int k = 0; k < 7; ++k) s[k] = 0.0;
        atomicAdd(&a.stats[0], 1u);
        return;
    }
    const double area = sqrt(ddot(nx, ny, nz, nx, ny, nz));
    s[0] = nx, s[1] = ny, s[2] = nz, s[3] = area;
    for (int j = 0; j < 3; ++j) s[4 + j] = area * (((p[0][j] + p[1][j]) + p[2][j]) / 3.0);
}

__global__ __launch_bounds__(kBlock) void k_wn_links(const float4* nodes, uint32_t n, uint32_t* parent)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i + 1u >= n) return;
    const float4 q = nodes[4 * (size_t)i + 3];
    const int    c[2] = {(int)f2u(q.z), (int)f2u(q.w)};
    for (uint32_t s = 0; s < 2u; ++s)
        if (c[s] >= 0 && (uint32_t)c[s] + 1u < n) parent[c[s]] = (i << 1) | s;
}

__global__ __launch_bounds__(kBlock) void k_wn_climb(WindingBuildArgs a)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x, n = a.tri_count;
    if (k >= 2u * (n - 1u)) return;
    uint32_t     node = k >> 1, slot = k & 1u;
    const float4 q    = a.nodes[4 * (size_t)node + 3];
    const int    c    = (int)f2u(slot ? q.w : q.z);
    if (c >= 0) return;  // an inner child: its sums arrive from below
    const uint32_t code = (uint32_t)~c, first = code & kLeafFirstMask, count = (code >> kLeafCountShift) + 1u;
    double         mine[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t t = first; t < first + count && t < n; ++t)
        for (int j = 0; j < 7; ++j) mine[j] += a.tri_sums[7 * (size_t)t + j];
    for (;;)
    {
        double* const s = a.sums + 14 * (size_t)node;
        for (int j = 0; j < 7; ++j) s[7 * slot + j] = mine[j];
        __threadfence();
        const uint32_t arrived = __hip_atomic_fetch_add(&a.flags[node], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == 0) return;
        __threadfence();
        // slot 0 + slot 1, whichever of the two this thread brought
        for (int j = 0; j < 7; ++j)
        {
            const double other = load_agent(s + 7 * (slot ^ 1u) + j);
            mine[j]            = slot ? other + mine[j] : mine[j] + other;
        }
        const uint32_t up = a.parent[node];
        if (up == kNoParent)
        {
            if (node == 0)
                for (int j = 0; j < 7; ++j) a.root[j] = mine[j];
            return;
        }
        node = up >> 1, slot = up & 1u;
    }
}

__global__ __launch_bounds__(kBlock) void k_wn_records(WindingBuildArgs a)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x, n = a.tri_count;
    if (k >= 2u * (n - 1u)) return;
    const uint32_t node = k >> 1, slot = k & 1u;
    const float*   q    = reinterpret_cast<const float*>(a.nodes + 4 * (size_t)node);
    const float*   box  = q + 6u * slot;  // (lo.xyz, hi.xyz) of the child as the tree stores it
    const double*  s    = a.sums + 14 * (size_t)node + 7u * slot;
    const double   area = s[3];
    float          pc[3];
    for (int j = 0; j < 3; ++j) pc[j] = area != 0.0 ? (float)(s[4 + j] / area) : (float)(0.5 * ((double)box[j] + (double)box[3 + j]));
    double far[3];
    for (int j = 0; j < 3; ++j) far[j] = fmax(fabs((double)box[j] - (double)pc[j]), fabs((double)box[3 + j] - (double)pc[j]));
    float r = (float)sqrt(ddot(far[0], far[1], far[2], far[0], far[1], far[2]));
    if (r >= 0.f && r < __builtin_inff()) r = u2f(f2u(r) + 1u);  // one ulp up: the ball is never too small
    float4* const out = a.table + 4 * (size_t)node + 2u * slot;
    out[0]            = make_float4(pc[0], pc[1], pc[2], r);
    out[1]            = make_float4((float)s[0], (float)s[1], (float)s[2], q[14 + slot]);
}

// ---- the walk ----
constexpr float kInv2Pi = 0.15915494f;  // fl(1 / (2 pi))
constexpr float k4Pi    = 12.566371f;   // fl(4 pi)

// Workgroups per CU: the stack is 4 B x STACK x kBlock of the CU's 160 KB of LDS, which allows 10, 6, 5 and 2; a CU holds 8 workgroups
// of four waves at most, and that leaves 64 VGPRs, which the walk fits without scratch (tools/kernel_regs.sh; DESIGN.md "Winding numbers")
constexpr int winding_blocks(int STACK) { return STACK <= 16 ? 8 : STACK <= 24 ? 6 : STACK <= 32 ? 5 : 2; }

// A child's dipole seen from p, all binary32 and unfused: far iff d2 > fl(fl(beta r)^2); then the first-order term
__device__ __forceinline__ bool winding_far(const float4 pr, const float4 nc, const float4 p, float beta, float& term)
{
    const float dx = pr.x - p.x, dy = pr.y - p.y, dz = pr.z - p.z;
    const float d2  = dot_c(dx, dy, dz, dx, dy, dz);
    const float lim = beta * pr.w;
    if (!(d2 > lim * lim)) return false;
    term = dot_c(nc.x, nc.y, nc.z, dx, dy, dz) / ((k4Pi * d2) * sqrtf(d2));
    return true;
}

// Van Oosterom & Strackee on the stored record (v0, e1, e2, n = fl(e1 x e2)): a = v0 - p, b = a + e1, c = a + e2, det = dot(a, n)
__device__ __forceinline__ float winding_exact(const float4 t0, const float4 t1, const float4 t2, const float4 p)
{
    const float ax = t0.x - p.x, ay = t0.y - p.y, az = t0.z - p.z;
    const float bx = ax + t0.w, by = ay + t1.x, bz = az + t1.y;
    const float cx = ax + t1.z, cy = ay + t1.w, cz = az + t2.x;
    const float la = sqrtf(dot_c(ax, ay, az, ax, ay, az)), lb = sqrtf(dot_c(bx, by, bz, bx, by, bz)), lc = sqrtf(dot_c(cx, cy, cz, cx, cy, cz));
    const float det = dot_c(ax, ay, az, t2.y, t2.z, t2.w);
    const float den = (((la * lb) * lc + dot_c(ax, ay, az, bx, by, bz) * lc) + dot_c(bx, by, bz, cx, cy, cz) * la) + dot_c(cx, cy, cz, ax, ay, az) * lb;
    return atan2f(det, den) * kInv2Pi;
}

// One lane per point, a grid-stride loop.  At a node the far terms of its two slots are added first, slot 0 then slot 1; then the near
// children are walked, slot 0's subtree before slot 1's (which waits as a node code in the lane's LDS column: at most one push per
// level, STACK at least the tree's depth).  A leaf adds the exact term of each of its triangles in leaf order; a NaN term (a record
// with a non-finite word) adds nothing.
template <int STACK>
__global__ __launch_bounds__(kBlock, winding_blocks(STACK)) void k_winding(BvhDev bvh, WindingArgs w)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < w.n; i += gridDim.x * kBlock)
    {
        const float4 p   = w.points[i];
        const float  inf = __builtin_inff();
        double       acc = 0.0;
        uint32_t     far = 0u, exact = 0u;
        const bool   ok  = fabsf(p.x) < inf && fabsf(p.y) < inf && fabsf(p.z) < inf;  // (a NaN fails its comparison)
        int          node = bvh.root, sp = 0;
        while (ok && bvh.tri_count != 0u)
        {
            if (node >= 0)
            {
                const float4* rec = w.table + 4 * (size_t)node;
                const float4  r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                float         t0 = 0.f, t1 = 0.f;
                const bool    f0 = winding_far(r0, r1, p, w.beta, t0), f1 = winding_far(r2, r3, p, w.beta, t1);
                if (f0) acc += (double)t0, ++far;
                if (f1) acc += (double)t1, ++far;
                const int c0 = (int)f2u(r1.w), c1 = (int)f2u(r3.w);
                if (!f0 && !f1)
                {
                    if (sp < STACK) stack[(sp++) * kBlock] = (uint32_t)c1;
                    node = c0;
                    continue;
                }
                if (!f0 || !f1)
                {
                    node = f0 ? c1 : c0;
                    continue;
                }
            }
            else
            {
                const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                for (uint32_t leaf = first; leaf <= last; ++leaf)
                {
                    const float t = winding_exact(bvh.tris[4 * (size_t)leaf + 0], bvh.tris[4 * (size_t)leaf + 1], bvh.tris[4 * (size_t)leaf + 2], p);
                    if (t == t) acc += (double)t;
                }
                exact += last - first + 1u;
            }
            if (sp == 0) break;
            node = (int)stack[(--sp) * kBlock];
        }
        w.out[i] = ok ? (float)acc : __builtin_nanf("");
        if (w.visits) w.visits[2 * (size_t)i] = far, w.visits[2 * (size_t)i + 1] = exact;
    }
}
}  // namespace

void launch_winding_build(hipStream_t stream, const WindingBuildArgs& a)
{
    const uint32_t n = a.tri_count;
    if (n == 0) return;
    (void)hipMemsetAsync(a.stats, 0, 2 * sizeof(uint32_t), stream);
    (void)hipMemsetAsync(a.root, 0, 7 * sizeof(double), stream);
    hipLaunchKernelGGL(k_wn_triangles, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
    if (n == 1)
    {
        // a root that is a leaf: no records; the totals are the triangle's
        (void)hipMemcpyAsync(a.root, a.tri_sums, 7 * sizeof(double), hipMemcpyDeviceToDevice, stream);
        return;
    }
    const uint32_t inner = n - 1u, slots = 2u * inner;
    (void)hipMemsetAsync(a.parent, 0xff, sizeof(uint32_t) * inner, stream);
    (void)hipMemsetAsync(a.flags, 0, sizeof(uint32_t) * inner, stream);
    (void)hipMemsetAsync(a.sums, 0, sizeof(double) * 14 * (size_t)inner, stream);
    hipLaunchKernelGGL(k_wn_links, dim3((inner + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a.nodes, n, a.parent);
    hipLaunchKernelGGL(k_wn_climb, dim3((slots + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
    hipLaunchKernelGGL(k_wn_records, dim3((slots + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
}

void launch_winding_numbers(const LaunchCfg& cfg, const BvhDev& bvh, const WindingArgs& a, uint32_t depth)
{
    with_stack_class(depth, [&](auto S) { launch_points<k_winding<decltype(S)::value>>(cfg, a.n, bvh, a); });
}
}  // namespace cap
