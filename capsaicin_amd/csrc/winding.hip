// winding.hip — generalised winding numbers (Jacobson et al. 2013) over the scene's binary tree, gfx950: the first-order dipole table of
// cap_winding_build (Barill et al. 2018), the walk of cap_winding_numbers and that of cap_winding_instances.  include/capsaicin_hip.h ("winding numbers") has the
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
//
// Over instances (cap_winding_instances; include/capsaicin_hip.h "winding numbers over instances", DESIGN.md "Winding numbers over
// instances"): the same build on an object's node and record range of the forest (WindingBuildArgs::node_base, rec_base, rec_ids), the
// derived tables (k_wi_instances: L, |det L|, sigma per instance; k_wi_top_leaves / k_wi_top_level: one world dipole per top-level
// entry, level by level in binary64) and the two-level walk k_winding_inst at the end of the file.
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
    const uint32_t g  = a.rec_ids ? f2u(a.rec_ids[4 * (size_t)i + 3].x) : a.leaf_tri[i];
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

// (node_base: what the child codes of an object's tree in the forest carry beyond the object's own numbering; 0 for the scene's)
__global__ __launch_bounds__(kBlock) void k_wn_links(const float4* nodes, uint32_t n, uint32_t node_base, uint32_t* parent)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i + 1u >= n) return;
    const float4 q = nodes[4 * (size_t)i + 3];
    const int    c[2] = {(int)f2u(q.z), (int)f2u(q.w)};
    for (uint32_t s = 0; s < 2u; ++s)
        if (c[s] >= 0 && (uint32_t)c[s] >= node_base && (uint32_t)c[s] - node_base + 1u < n) parent[(uint32_t)c[s] - node_base] = (i << 1) | s;
}

__global__ __launch_bounds__(kBlock) void k_wn_climb(WindingBuildArgs a)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x, n = a.tri_count;
    if (k >= 2u * (n - 1u)) return;
    uint32_t     node = k >> 1, slot = k & 1u;
    const float4 q    = a.nodes[4 * (size_t)node + 3];
    const int    c    = (int)f2u(slot ? q.w : q.z);
    if (c >= 0) return;  // an inner child: its sums arrive from below
    const uint32_t code = (uint32_t)~c, first = (code & kLeafFirstMask) - a.rec_base, count = (code >> kLeafCountShift) + 1u;
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
// ---- winding numbers over instances (cap_winding_instances): the derived tables ----
// One thread per instance: L, |det L| and sigma >= ||L||_2 of the descriptor's linear part, in binary64 and rounded once.  sigma =
// sqrt(||L||_1 ||L||_inf) rounded up: exactly 1 for the identity.  An instance contributes iff its record's mask word is not 0 (0 for an
// inert one) and its determinant is a finite number that is not 0.
__global__ __launch_bounds__(kBlock) void k_wi_instances(WindingInstBuildArgs a)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const float4 m0 = a.descs[4 * (size_t)i], m1 = a.descs[4 * (size_t)i + 1], m2 = a.descs[4 * (size_t)i + 2];
    const float  lf[9] = {m0.x, m0.y, m0.z, m1.x, m1.y, m1.z, m2.x, m2.y, m2.z};
    double       l[9];
    for (int k = 0; k < 9; ++k) l[k] = (double)lf[k];
    const double det = (l[0] * (l[4] * l[8] - l[5] * l[7]) - l[1] * (l[3] * l[8] - l[5] * l[6])) + l[2] * (l[3] * l[7] - l[4] * l[6]);
    double       n1 = 0.0, ninf = 0.0;
    for (int k = 0; k < 3; ++k)
    {
        n1   = fmax(n1, (fabs(l[k]) + fabs(l[3 + k])) + fabs(l[6 + k]));
        ninf = fmax(ninf, (fabs(l[3 * k]) + fabs(l[3 * k + 1])) + fabs(l[3 * k + 2]));
    }
    const double sg  = sqrt(n1 * ninf);
    float        sig = (float)sg;
    if ((double)sig < sg) sig = u2f(f2u(sig) + 1u);
    const float    ad   = (float)fabs(det);
    const uint32_t mask = f2u(a.rec[4 * (size_t)i + 3].x) & 0xFFu;
    const bool     on   = mask != 0u && det != 0.0 && ad < __builtin_inff() && sig < __builtin_inff();  // (a NaN fails its comparison)
    a.inst[3 * (size_t)i + 0] = make_float4(lf[0], lf[1], lf[2], lf[3]);
    a.inst[3 * (size_t)i + 1] = make_float4(lf[4], lf[5], lf[6], lf[7]);
    a.inst[3 * (size_t)i + 2] = make_float4(lf[8], ad, sig, on ? (det < 0.0 ? -1.f : 1.f) : 0.f);
    if (on) atomicAdd(a.count, 1u);
}

__device__ __forceinline__ void wi_store_empty(float4* e, uint32_t word7)
{
    e[0] = make_float4(0.f, 0.f, 0.f, -1.f);
    e[1] = make_float4(0.f, 0.f, 0.f, u2f(word7));
}

// (p~_w, r) (N_w, word 7) of an entry from its sums and its stored world box: the scene table's rule (k_wn_records)
__device__ __forceinline__ void wi_store_entry(float4* e, const double* s, const float4 lo, const float4 hi, uint32_t word7)
{
    const float  box[6] = {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z};
    const double w      = s[3];
    float        pc[3];
    for (int j = 0; j < 3; ++j) pc[j] = w != 0.0 ? (float)(s[4 + j] / w) : (float)(0.5 * ((double)box[j] + (double)box[3 + j]));
    double far[3];
    for (int j = 0; j < 3; ++j) far[j] = fmax(fabs((double)box[j] - (double)pc[j]), fabs((double)box[3 + j] - (double)pc[j]));
    float r = (float)sqrt(ddot(far[0], far[1], far[2], far[0], far[1], far[2]));
    if (r >= 0.f && r < __builtin_inff()) r = u2f(f2u(r) + 1u);
    e[0] = make_float4(pc[0], pc[1], pc[2], r);
    e[1] = make_float4((float)s[0], (float)s[1], (float)s[2], u2f(word7));
}

// Level 0, entry j = the instance the TLAS holds there: N_w = s cof(L) N, p~_w = M p~, weight A |det L|^(2/3), from the root sums of the
// instance's object.  Entries of instances that do not contribute, and the padding entry, are empty.
__global__ __launch_bounds__(kBlock) void k_wi_top_leaves(WindingInstBuildArgs a)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= a.n + (a.n & 1u)) return;
    double* const s = a.top_sums + 7 * (size_t)j;
    float4* const e = a.top + 2 * (size_t)j;
    const float4  lo = a.tlas[2 * (size_t)j], hi = a.tlas[2 * (size_t)j + 1];
    const uint32_t i  = f2u(hi.w);
    const float    sn = j < a.n && i < a.n ? a.inst[3 * (size_t)i + 2].w : 0.f;
    if (sn == 0.f || !(lo.w >= 0.f))
    {
        for (int k = 0; k < 7; ++k) s[k] = 0.0;
        wi_store_empty(e, j < a.n ? i : kInvalidId);
        return;
    }
    const float4  m0 = a.descs[4 * (size_t)i], m1 = a.descs[4 * (size_t)i + 1], m2 = a.descs[4 * (size_t)i + 2];
    const double  m[12] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w};
    const double* o  = a.obj_root + 7 * (size_t)f2u(a.rec[4 * (size_t)i + 3].z);
    const double  sd = (double)sn;
    // cof(L): row r is the cross product of the two other rows of L
    const double c[9] = {m[5] * m[10] - m[6] * m[9], m[6] * m[8] - m[4] * m[10], m[4] * m[9] - m[5] * m[8],
                         m[9] * m[2] - m[10] * m[1], m[10] * m[0] - m[8] * m[2], m[8] * m[1] - m[9] * m[0],
                         m[1] * m[6] - m[2] * m[5],  m[2] * m[4] - m[0] * m[6],  m[0] * m[5] - m[1] * m[4]};
    for (int r = 0; r < 3; ++r) s[r] = sd * ddot(c[3 * r], c[3 * r + 1], c[3 * r + 2], o[0], o[1], o[2]);
    const double det = ddot(m[0], m[1], m[2], c[0], c[1], c[2]);
    const double w   = o[3] * cbrt(det * det);
    s[3]             = w;
    for (int r = 0; r < 3; ++r)
    {
        const double pr = o[3] != 0.0 ? ddot(m[4 * r], m[4 * r + 1], m[4 * r + 2], o[4] / o[3], o[5] / o[3], o[6] / o[3]) + m[4 * r + 3] : 0.0;
        s[4 + r]        = w * pr;
    }
    wi_store_entry(e, s, lo, hi, i);
}

// One level from the one below, in k_tlas_level's layout: entry j = entry 2 j + entry 2 j + 1, in binary64 and in that order
__global__ __launch_bounds__(kBlock) void k_wi_top_level(WindingInstBuildArgs a, uint32_t src, uint32_t dst, uint32_t n_dst)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_dst + (n_dst & 1u)) return;
    double* const s = a.top_sums + 7 * (size_t)(dst + j);
    float4* const e = a.top + 2 * (size_t)(dst + j);
    const bool    v0 = j < n_dst && a.top[2 * (size_t)(src + 2u * j)].w >= 0.f, v1 = j < n_dst && a.top[2 * (size_t)(src + 2u * j + 1u)].w >= 0.f;
    if (!v0 && !v1)
    {
        for (int k = 0; k < 7; ++k) s[k] = 0.0;
        wi_store_empty(e, kInvalidId);
        return;
    }
    const double* s0 = a.top_sums + 7 * (size_t)(src + 2u * j);
    for (int k = 0; k < 7; ++k) s[k] = s0[k] + s0[7 + k];  // (an empty entry's sums are zeros)
    wi_store_entry(e, s, a.tlas[2 * (size_t)(dst + j)], a.tlas[2 * (size_t)(dst + j) + 1], kInvalidId);
}

// ---- winding numbers over instances: the walk ----
struct WiInst  // what the object walk keeps of the instance it is in
{
    float l[9], det, sigma;
};
__device__ __forceinline__ void wi_world(const WiInst& t, float x, float y, float z, float& wx, float& wy, float& wz)
{
    wx = dot_c(t.l[0], t.l[1], t.l[2], x, y, z), wy = dot_c(t.l[3], t.l[4], t.l[5], x, y, z), wz = dot_c(t.l[6], t.l[7], t.l[8], x, y, z);
}

// winding_far below an instance: the object-space dipole seen from p' = W q, measured in world space through d_w = L d'.  The world ball
// of radius sigma r covers the image of the object-space ball; the world area vector is cof(L) N, and the cofactor cancels against L d'.
__device__ __forceinline__ bool winding_far_inst(const float4 pr, const float4 nc, const float4 p, const WiInst& t, float beta, float& term)
{
    const float dx = pr.x - p.x, dy = pr.y - p.y, dz = pr.z - p.z;
    float       wx, wy, wz;
    wi_world(t, dx, dy, dz, wx, wy, wz);
    const float d2  = dot_c(wx, wy, wz, wx, wy, wz);
    const float lim = beta * (t.sigma * pr.w);
    if (!(d2 > lim * lim)) return false;
    term = (t.det * dot_c(nc.x, nc.y, nc.z, dx, dy, dz)) / ((k4Pi * d2) * sqrtf(d2));
    return true;
}

// winding_exact below an instance: lengths and dots of the world corners L a', L b', L c'; s det_w = |det L| dot(a', n)
__device__ __forceinline__ float winding_exact_inst(const float4 t0, const float4 t1, const float4 t2, const float4 p, const WiInst& t)
{
    const float ox = t0.x - p.x, oy = t0.y - p.y, oz = t0.z - p.z;
    float       ax, ay, az, bx, by, bz, cx, cy, cz;
    wi_world(t, ox, oy, oz, ax, ay, az);
    wi_world(t, ox + t0.w, oy + t1.x, oz + t1.y, bx, by, bz);
    wi_world(t, ox + t1.z, oy + t1.w, oz + t2.x, cx, cy, cz);
    const float la = sqrtf(dot_c(ax, ay, az, ax, ay, az)), lb = sqrtf(dot_c(bx, by, bz, bx, by, bz)), lc = sqrtf(dot_c(cx, cy, cz, cx, cy, cz));
    const float det = t.det * dot_c(ox, oy, oz, t2.y, t2.z, t2.w);
    const float den = (((la * lb) * lc + dot_c(ax, ay, az, bx, by, bz) * lc) + dot_c(bx, by, bz, cx, cy, cz) * la) + dot_c(cx, cy, cz, ax, ay, az) * lb;
    return atan2f(det, den) * kInv2Pi;
}

// Workgroups per CU: the LDS slice (the stack and the 104 bytes of level offsets) allows 9, 6, 4 and 2; the instance's L, |det L| and
// sigma, p' and the top-level state take the walk to 71 VGPRs, which seven workgroups of four waves still hold without scratch
// (tools/kernel_regs.sh; DESIGN.md "Winding numbers over instances")
constexpr int winding_inst_blocks(int STACK) { return STACK <= 16 ? 7 : STACK <= 24 ? 6 : STACK <= 32 ? 4 : 2; }

// One lane per point, a grid-stride loop, one loop with three kinds of step as k_query_inst (instance.hip), so that the lanes of a wave
// that are at the top level advance while others are inside an instance:
//   * a top-level node (level, idx) of the implicit tree, without a stack: the far terms of its two entries are added, slot 0 then slot
//     1, by winding_far on the world dipole; then the near entries are entered, slot 0's subtree first (`pending` holds one bit per
//     level where slot 1 is still owed).  At level 1 the near entries are instances and wait in (todo0, todo1).  An empty entry (r < 0)
//     is neither far nor near;
//   * entering an instance: p' = W q by the point queries' formula; a degenerate p' leaves the instance out;
//   * a node or leaf of the object's tree: k_winding's walk with winding_far_inst / winding_exact_inst.
// visits: the far terms of the top level, the instances entered, the far terms below instances, the exact triangles.
template <int STACK>
__global__ __launch_bounds__(kBlock, winding_inst_blocks(STACK)) void k_winding_inst(BvhDev bvh, WindingInstArgs wa, TlasDev tl)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    __shared__ uint32_t lds_off[kTlasMaxLevels + 1];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    if (threadIdx.x <= tl.top) lds_off[threadIdx.x] = tl.level_off[threadIdx.x];
    __syncthreads();
    const WindingArgs& w = wa.a;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < w.n; i += gridDim.x * kBlock)
    {
        const float4 q   = w.points[i];
        const float  inf = __builtin_inff();
        double       acc = 0.0;
        uint32_t     far_top = 0u, entered = 0u, far = 0u, exact = 0u;
        const bool   ok = fabsf(q.x) < inf && fabsf(q.y) < inf && fabsf(q.z) < inf;  // (a NaN fails its comparison)
        uint32_t     level = tl.top + 1u, idx = 0u, pending = 0u, todo0 = kInvalidId, todo1 = kInvalidId;
        bool         done = false, in_obj = false;
        WiInst       t{};
        float4       p = q;  // p' inside an instance
        int          node = 0, sp = 0;
        while (ok && bvh.tri_count != 0u)
        {
            if (in_obj)
            {
                if (node >= 0)
                {
                    const float4* rec = w.table + 4 * (size_t)node;
                    const float4  r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                    float         t0 = 0.f, t1 = 0.f;
                    const bool    f0 = winding_far_inst(r0, r1, p, t, w.beta, t0), f1 = winding_far_inst(r2, r3, p, t, w.beta, t1);
                    if (f0) acc += t0 == t0 ? (double)t0 : 0.0, ++far;
                    if (f1) acc += t1 == t1 ? (double)t1 : 0.0, ++far;
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
                        const float v = winding_exact_inst(bvh.tris[4 * (size_t)leaf + 0], bvh.tris[4 * (size_t)leaf + 1], bvh.tris[4 * (size_t)leaf + 2], p, t);
                        if (v == v) acc += (double)v;
                    }
                    exact += last - first + 1u;
                }
                if (sp == 0)
                    in_obj = false;
                else
                    node = (int)stack[(--sp) * kBlock];
                continue;
            }
            if (todo0 != kInvalidId)
            {
                const uint32_t inst = todo0;
                todo0 = todo1, todo1 = kInvalidId;
                const float4 w0 = tl.rec[4 * (size_t)inst], w1 = tl.rec[4 * (size_t)inst + 1], w2 = tl.rec[4 * (size_t)inst + 2];
                p.x = (dot_c(w0.x, w0.y, w0.z, q.x, q.y, q.z)) + w0.w;
                p.y = (dot_c(w1.x, w1.y, w1.z, q.x, q.y, q.z)) + w1.w;
                p.z = (dot_c(w2.x, w2.y, w2.z, q.x, q.y, q.z)) + w2.w;
                if (!(fabsf(p.x) < inf && fabsf(p.y) < inf && fabsf(p.z) < inf)) continue;
                const float4 l0 = wa.inst[3 * (size_t)inst], l1 = wa.inst[3 * (size_t)inst + 1], l2 = wa.inst[3 * (size_t)inst + 2];
                t.l[0] = l0.x, t.l[1] = l0.y, t.l[2] = l0.z, t.l[3] = l0.w, t.l[4] = l1.x, t.l[5] = l1.y, t.l[6] = l1.z, t.l[7] = l1.w, t.l[8] = l2.x;
                t.det = l2.y, t.sigma = l2.z;
                node  = (int)f2u(tl.rec[4 * (size_t)inst + 3].y);
                sp = 0, in_obj = true, ++entered;
                continue;
            }
            if (done) break;
            // a top-level node: its two entries
            const float4* e = wa.top + 2 * (size_t)(lds_off[level - 1u] + 2u * idx);
            const float4  r0 = e[0], r1 = e[1], r2 = e[2], r3 = e[3];
            float         t0 = 0.f, t1 = 0.f;
            const bool    f0 = r0.w >= 0.f && winding_far(r0, r1, q, w.beta, t0), f1 = r2.w >= 0.f && winding_far(r2, r3, q, w.beta, t1);
            if (f0) acc += t0 == t0 ? (double)t0 : 0.0, ++far_top;
            if (f1) acc += t1 == t1 ? (double)t1 : 0.0, ++far_top;
            const bool n0 = r0.w >= 0.f && !f0, n1 = r2.w >= 0.f && !f1;
            if (level > 1u)
            {
                if (n0 || n1)
                {
                    if (n0 && n1) pending |= 1u << (level - 1u);
                    idx   = 2u * idx + (n0 ? 0u : 1u);
                    level = level - 1u;
                    continue;
                }
            }
            else if (n0 || n1)
            {
                const uint32_t i0 = f2u(r1.w), i1 = f2u(r3.w);
                todo0 = n0 ? i0 : i1, todo1 = n0 && n1 ? i1 : kInvalidId;
            }
            const uint32_t owed = pending >> level;
            if (owed == 0u)
            {
                done = true;
                continue;
            }
            const uint32_t up = (uint32_t)__builtin_ctz(owed);
            idx     = (idx >> up) ^ 1u;
            level   = level + up;
            pending = pending & ~(1u << level);
        }
        w.out[i] = ok ? (float)acc : __builtin_nanf("");
        if (w.visits)
        {
            uint32_t* const v = w.visits + 4 * (size_t)i;
            v[0] = far_top, v[1] = entered, v[2] = far, v[3] = exact;
        }
    }
}
}  // namespace

void launch_winding_instances_build(hipStream_t stream, const WindingInstBuildArgs& a)
{
    const uint32_t n = a.n;
    if (n == 0) return;
    (void)hipMemsetAsync(a.count, 0, sizeof(uint32_t), stream);
    hipLaunchKernelGGL(k_wi_instances, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
    uint32_t       off[kTlasMaxLevels];
    const uint32_t top = tlas_layout(n, off, nullptr);
    hipLaunchKernelGGL(k_wi_top_leaves, dim3((n + 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
    uint32_t cnt = n;
    for (uint32_t l = 1; l <= top; ++l)  // one level per launch, in k_tlas_level's order
    {
        const uint32_t next = (cnt + 1u) / 2u;
        hipLaunchKernelGGL(k_wi_top_level, dim3((next + 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a, off[l - 1], off[l], next);
        cnt = next;
    }
}

void launch_winding_instances(const LaunchCfg& cfg, const BvhDev& bvh, const WindingInstArgs& a, const TlasDev& tl, uint32_t depth)
{
    with_stack_class(depth, [&](auto S) { launch_points<k_winding_inst<decltype(S)::value>>(cfg, a.a.n, bvh, a, tl); });
}

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
    hipLaunchKernelGGL(k_wn_links, dim3((inner + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a.nodes, n, a.node_base, a.parent);
    hipLaunchKernelGGL(k_wn_climb, dim3((slots + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
    hipLaunchKernelGGL(k_wn_records, dim3((slots + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
}

void launch_winding_numbers(const LaunchCfg& cfg, const BvhDev& bvh, const WindingArgs& a, uint32_t depth)
{
    with_stack_class(depth, [&](auto S) { launch_points<k_winding<decltype(S)::value>>(cfg, a.n, bvh, a); });
}
}  // namespace cap
