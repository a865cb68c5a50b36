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
//
// Each step stands once (DESIGN.md "Winding numbers", "One copy of each step"):
//   dipole_record                    (p~, r) (N, word 7) from sums and a stored box: k_wn_records, k_wi_top_leaves, k_wi_top_level
//   winding_far<M>, winding_exact<M> the two terms in the metric M of the walk: WnFlat (nothing to map) or WiInst (L, |det L|, sigma)
//   winding_node_step<STACK, M>      an inner node: two far tests, the far terms slot 0 then slot 1, push / descend
//   winding_leaf_step<M>             a leaf's exact terms in leaf order
//   winding_top_step                 a top-level node over instances; its tail is top_advance, the pop ray_pop (cap_query_walk.h)
// k_winding is node step, leaf step and pop in WnFlat; k_winding_inst is the top step, the entry into an instance and the same three in WiInst.
#include "cap_kernels.h"
#include "cap_leaf.h"
#include "cap_query_walk.h"  // with_stack_class, launch_points

namespace cap
{
namespace
{
constexpr uint32_t kNoParent = 0xffffffffu;

// dot of the contract (dot_c: cap_query_walk.h) in double: no fused multiply-add (the build has -ffp-contract=off)
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

// The record rule, for the scene's and objects' tables and for the top level over instances: (p~, r) (N, word 7) from the sums
// (N, weight, weight x centre) and the stored box (lo.xyz, hi.xyz).  p~ is the binary64 quotient rounded once to binary32, or the box
// centre where the weight is 0; r is measured from that ROUNDED p~ to the farthest corner and stepped one ulp up.
__device__ __forceinline__ void dipole_record(float4* out, const double* s, const float* box, const float& word7)
{
    const double w = s[3];
    float        pc[3];
    for (int j = 0; j < 3; ++j) pc[j] = w != 0.0 ? (float)(s[4 + j] / w) : (float)(0.5 * ((double)box[j] + (double)box[3 + j]));
    double far[3];
    for (int j = 0; j < 3; ++j) far[j] = fmax(fabs((double)box[j] - (double)pc[j]), fabs((double)box[3 + j] - (double)pc[j]));
    float r = (float)sqrt(ddot(far[0], far[1], far[2], far[0], far[1], far[2]));
    if (r >= 0.f && r < __builtin_inff()) r = u2f(f2u(r) + 1u);  // one ulp up: the ball is never too small
    out[0] = make_float4(pc[0], pc[1], pc[2], r);
    out[1] = make_float4((float)s[0], (float)s[1], (float)s[2], word7);
}

__global__ __launch_bounds__(kBlock) void k_wn_records(WindingBuildArgs a)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x, n = a.tri_count;
    if (k >= 2u * (n - 1u)) return;
    const uint32_t node = k >> 1, slot = k & 1u;
    const float*   q    = reinterpret_cast<const float*>(a.nodes + 4 * (size_t)node);
    // (the child's box as the tree stores it, its sums, its code)
    dipole_record(a.table + 4 * (size_t)node + 2u * slot, a.sums + 14 * (size_t)node + 7u * slot, q + 6u * slot, q[14 + slot]);
}

// ---- the walk ----
constexpr float kInv2Pi = 0.15915494f;  // fl(1 / (2 pi))
constexpr float k4Pi    = 12.566371f;   // fl(4 pi)

// Workgroups per CU: the stack is 4 B x STACK x kBlock of the CU's 160 KB of LDS, which allows 10, 6, 5 and 2; a CU holds 8 workgroups
// of four waves at most, and that leaves 64 VGPRs, which the walk fits without scratch (tools/kernel_regs.sh; DESIGN.md "Winding numbers")
constexpr int winding_blocks(int STACK) { return STACK <= 16 ? 8 : STACK <= 24 ? 6 : STACK <= 32 ? 5 : 2; }

// ---- the steps of both walks, each once (DESIGN.md "Winding numbers", "One copy of each step") ----
// The metric a walk measures its terms in.  kMapped: differences go through L before lengths and dots are taken, radii through sigma,
// numerators through |det L|; without it `if constexpr` leaves none of that behind.  kGuardFar: a NaN FAR term adds nothing
// (cap_winding_instances, at the top level and below an instance) or is added and makes the result NaN (cap_winding_numbers): the two
// contracts differ as they were written and this file keeps both.  A NaN EXACT term adds nothing in either.
struct WnFlat  // the scene's own space: nothing to map
{
    static constexpr bool kMapped = false, kGuardFar = false;
};
struct WiInst  // below an instance: what the object walk keeps of the instance it is in
{
    static constexpr bool kMapped = true, kGuardFar = true;
    float                 l[9], det, sigma;
};
__device__ __forceinline__ void wi_world(const WiInst& t, float x, float y, float z, float& wx, float& wy, float& wz)
{
    wx = dot_c(t.l[0], t.l[1], t.l[2], x, y, z), wy = dot_c(t.l[3], t.l[4], t.l[5], x, y, z), wz = dot_c(t.l[6], t.l[7], t.l[8], x, y, z);
}

// A child's dipole seen from p, all binary32 and unfused: far iff d2 > fl(fl(beta r)^2); then the first-order term.  Below an instance
// p = p' = W q and the object-space dipole is measured in world space through d_w = L d': the world ball of radius sigma r covers the
// image of the object-space ball; the world area vector is cof(L) N, and the cofactor cancels against L d'.
template <typename M>
__device__ __forceinline__ bool winding_far(const float4 pr, const float4 nc, const float4 p, const M& m, float beta, float& term)
{
    const float dx = pr.x - p.x, dy = pr.y - p.y, dz = pr.z - p.z;
    float       wx = dx, wy = dy, wz = dz, r = pr.w;
    if constexpr (M::kMapped) wi_world(m, dx, dy, dz, wx, wy, wz), r = m.sigma * pr.w;
    const float d2  = dot_c(wx, wy, wz, wx, wy, wz);
    const float lim = beta * r;
    if (!(d2 > lim * lim)) return false;
    float num = dot_c(nc.x, nc.y, nc.z, dx, dy, dz);
    if constexpr (M::kMapped) num = m.det * num;
    term = num / ((k4Pi * d2) * sqrtf(d2));
    return true;
}

// Van Oosterom & Strackee on the stored record (v0, e1, e2, n = fl(e1 x e2)): a = v0 - p, b = a + e1, c = a + e2, det = dot(a, n).
// Below an instance the lengths and dots are those of the world corners L a, L b, L c, and s det_w = |det L| dot(a, n).
template <typename M>
__device__ __forceinline__ float winding_exact(const float4 t0, const float4 t1, const float4 t2, const float4 p, const M& m)
{
    const float ox = t0.x - p.x, oy = t0.y - p.y, oz = t0.z - p.z;
    float       ax = ox, ay = oy, az = oz;
    float       bx = ox + t0.w, by = oy + t1.x, bz = oz + t1.y;
    float       cx = ox + t1.z, cy = oy + t1.w, cz = oz + t2.x;
    if constexpr (M::kMapped) wi_world(m, ax, ay, az, ax, ay, az), wi_world(m, bx, by, bz, bx, by, bz), wi_world(m, cx, cy, cz, cx, cy, cz);
    const float la = sqrtf(dot_c(ax, ay, az, ax, ay, az)), lb = sqrtf(dot_c(bx, by, bz, bx, by, bz)), lc = sqrtf(dot_c(cx, cy, cz, cx, cy, cz));
    float       det = dot_c(ox, oy, oz, t2.y, t2.z, t2.w);
    if constexpr (M::kMapped) det = m.det * det;
    const float den = (((la * lb) * lc + dot_c(ax, ay, az, bx, by, bz) * lc) + dot_c(bx, by, bz, cx, cy, cz) * la) + dot_c(cx, cy, cz, ax, ay, az) * lb;
    return atan2f(det, den) * kInv2Pi;
}

// A far term joins the sum by the rule of the walk G it was taken in
template <typename G>
__device__ __forceinline__ void winding_add_far(double& acc, float term)
{
    if constexpr (G::kGuardFar)
        acc += term == term ? (double)term : 0.0;
    else
        acc += (double)term;
}

// An inner node of a dipole table: the far terms of its two slots are added first, slot 0 then slot 1; then the near children are
// walked, slot 0's subtree before slot 1's (which waits as a node code in the lane's LDS column: at most one push per level, STACK at
// least the tree's depth; the guard drops a push beyond it).  true: both are far, the caller pops.  node and sp cross by reference;
// the leaf step takes and returns the sum by value (through a reference it cost k_winding 2 VGPRs).
template <int STACK, typename M>
__device__ __forceinline__ bool winding_node_step(const float4* table, const float4 p, const M& m, float beta, uint32_t* stack, double& acc, uint32_t& far,
                                                  int& node, int& sp)
{
    const float4* rec = table + 4 * (size_t)node;
    const float4  r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    float         t0 = 0.f, t1 = 0.f;
    const bool    f0 = winding_far(r0, r1, p, m, beta, t0), f1 = winding_far(r2, r3, p, m, beta, t1);
    if (f0) winding_add_far<M>(acc, t0), ++far;
    if (f1) winding_add_far<M>(acc, t1), ++far;
    const int c0 = (int)f2u(r1.w), c1 = (int)f2u(r3.w);
    if (!f0 && !f1)
    {
        if (sp < STACK) stack[(sp++) * kBlock] = (uint32_t)c1;
        node = c0;
        return false;
    }
    if (!f0 || !f1)
    {
        node = f0 ? c1 : c0;
        return false;
    }
    return true;
}

// A leaf: the exact term of each of its triangles in leaf order; a NaN term (a record with a non-finite word) adds nothing
template <typename M>
__device__ __forceinline__ double winding_leaf_step(const float4* tris, int node, const float4 p, const M& m, double acc, uint32_t& exact)
{
    const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
    for (uint32_t leaf = first; leaf <= last; ++leaf)
    {
        const float t = winding_exact(tris[4 * (size_t)leaf + 0], tris[4 * (size_t)leaf + 1], tris[4 * (size_t)leaf + 2], p, m);
        if (t == t) acc += (double)t;
    }
    exact += last - first + 1u;
    return acc;
}

// One lane per point, a grid-stride loop over winding_node_step, winding_leaf_step and the pop.  (The pop is ray_pop's body: called
// as ray_pop it gives this kernel another block layout and a 46th VGPR; k_winding_inst calls it.)
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
                if (!winding_node_step<STACK>(w.table, p, WnFlat{}, w.beta, stack, acc, far, node, sp)) continue;
            }
            else
                acc = winding_leaf_step(bvh.tris, node, p, WnFlat{}, acc, exact);
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

// (p~_w, r) (N_w, word 7) of an entry from its sums and its stored world box
__device__ __forceinline__ void wi_store_entry(float4* e, const double* s, const float4 lo, const float4 hi, uint32_t word7)
{
    const float box[6] = {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z};
    dipole_record(e, s, box, u2f(word7));
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
// Workgroups per CU: the LDS slice (the stack and the 104 bytes of level offsets) allows 9, 6, 4 and 2; the instance's L, |det L| and
// sigma, p' and the top-level state take the walk to 71 VGPRs, which seven workgroups of four waves still hold without scratch
// (tools/kernel_regs.sh; DESIGN.md "Winding numbers over instances")
constexpr int winding_inst_blocks(int STACK) { return STACK <= 16 ? 7 : STACK <= 24 ? 6 : STACK <= 32 ? 4 : 2; }

// One top-level node (TopWalk, cap_query_walk.h; the queue's two distance words are not used): the far terms of its two entries are
// added, slot 0 then slot 1, by winding_far on the world dipole; the near entries are what top_advance descends into, slot 0's subtree
// first, or queues as instances at level 1.  An empty entry (r < 0) is neither far nor near.
__device__ __forceinline__ TopWalk winding_top_step(const float4* top, const uint32_t* lds_off, const float4 q, float beta, double& acc, uint32_t& far_top,
                                                    TopWalk t)
{
    const float4* e = top + 2 * (size_t)(lds_off[t.level - 1u] + 2u * t.idx);
    const float4  r0 = e[0], r1 = e[1], r2 = e[2], r3 = e[3];
    float         t0 = 0.f, t1 = 0.f;
    const bool    f0 = r0.w >= 0.f && winding_far(r0, r1, q, WnFlat{}, beta, t0), f1 = r2.w >= 0.f && winding_far(r2, r3, q, WnFlat{}, beta, t1);
    if (f0) winding_add_far<WiInst>(acc, t0), ++far_top;
    if (f1) winding_add_far<WiInst>(acc, t1), ++far_top;
    return top_advance(t, r0.w >= 0.f && !f0, r2.w >= 0.f && !f1, false, f2u(r1.w), f2u(r3.w), 0.f, 0.f);
}

// One lane per point, a grid-stride loop, one loop with three kinds of step as k_query_inst (instance.hip), so that the lanes of a wave
// that are at the top level advance while others are inside an instance:
//   * a top-level node (winding_top_step);
//   * entering the instance at the head of the queue: p' = W q by the point queries' formula; a degenerate p' leaves the instance out;
//   * a node or leaf of the object's tree: k_winding's steps in the instance's metric.
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
        TopWalk      top = top_start(tl);
        bool         in_obj = false;
        WiInst       t{};
        float4       p = q;  // p' inside an instance
        int          node = 0, sp = 0;
        while (ok && bvh.tri_count != 0u)
        {
            if (in_obj)
            {
                if (node >= 0)
                {
                    if (!winding_node_step<STACK>(w.table, p, t, w.beta, stack, acc, far, node, sp)) continue;
                }
                else
                    acc = winding_leaf_step(bvh.tris, node, p, t, acc, exact);
                in_obj = ray_pop(stack, sp, node);
                continue;
            }
            if (top.todo0 != kInvalidId)
            {
                const uint32_t inst = top.todo0;
                top                 = top_pop(top);
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
            if (top.done) break;
            top = winding_top_step(wa.top, lds_off, q, w.beta, acc, far_top, top);
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
