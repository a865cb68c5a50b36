// instance.hip — instanced ray queries (cap_instances_set, cap_trace_instances, cap_trace_instances_occlusion, cap_trace_instances_multi), gfx950.
//
// Bottom-level structures -- the uploaded scene and its binary tree, or the objects of cap_objects_set (mesh ranges of the scene, one
// binary tree each in a forest laid out as the scene's tree), read as object space -- and a table of N instances, each with an
// object-to-world transform, a mask and the index of the object it shows.  This file holds the per-instance setup (inverse,
// conditioning, world box: fp64 on the device, so device descriptors never travel to the host), the top-level tree over the world boxes,
// the two-level query kernels (made of four steps, each written once: ray_top_step and ray_enter_instance below, ray_node_step and
// ray_pop of cap_query_walk.h) and the relocation of an object's tree into the forest.  Below, "object" is the instance's object:
// without an object table the one object is the scene.
//
// Hit set (include/capsaicin_hip.h): defined from the STORED W = fl32(inverse(M)) and the rounded object-space ray
// o' = fl(W o + W_t), d' = fl(W d) alone; the closest record is the minimum in (t, instance, triangle) order.  Boxes never decide:
//   * below an instance the walk is the binary tree's with `slab` on the object-space ray: the walk k_query_binary_f does on a
//     caller's ray, conservative for the ray it is given wherever its origin lies.  (The wide view's padding assumes origins within
//     4 M of the scene, query.hip; an object-space origin is usually far outside that, so the wide view is not used here.)
//   * the top level sees the WORLD ray, which is not the image of the rounded object-space ray.  With A = inverse(W) (exact), the image
//     of the object-space point o' + t d' is  o + t d + A (do + t dd),  do, dd the rounding errors of the twelve dot products:
//       |do| <= g4 (|W| |o| + |W_t|),  |dd| <= g3 |W| |d|   (g_k = k eps / (1 - k eps), eps = 2^-24; row-sum norms throughout)
//     so the world ray passes within  e(t) <= g4 kappa (|o| + t |d|) + g4 |A| |W_t|,  kappa = |A| |W|,  of the image of every
//     object-space point it reports a hit at.  Such a point lies in the object box B (the object's bounds + twice the build's leaf
//     padding, ctx_bvh.hip object_box), its image in the box of A(B)'s corners, so |o + t d| <= X + e(t), X the largest |coordinate| of that box, and
//     t |d| <= |o| + X + e(t):   e(t) <= (g4 kappa (2 |o| + X) + g4 |A| |W_t|) / (1 - g4 kappa).
//     Per world axis r the same holds with the row sum |A_r| in place of |A| (component r of A v is at most |A_r| |v|):
//       e_r(t) <= (g4 kappa_r (2 |o| + X) + g4 |A_r| |W_t|) / (1 - g4 kappa),  kappa_r = |A_r| |W| <= kappa,
//     so a transform that stretches one axis does not pad the others with that axis' error.
//     The part that does not depend on the ray goes into the stored box (k_instance_setup: pad_r = c eps (kappa_r X + |A_r| |W_t|)
//     + 4 eps X per axis, then rounded outwards), the part that does into tlas_slab: every box is inflated by k |o| per ray, k = 2 c eps kappa the
//     largest of its subtree.  c = kInstSlack = 32, eight times g4 / eps: the rest covers the float evaluation of the inflated
//     planes (2 eps (X + k |o|)), 1 / (1 - g4 kappa) <= 1.001 and the distance-proportional error of the triangle test itself, for
//     kappa <= CAP_INSTANCE_MAX_CONDITION = 4096, the domain of the proof; an instance beyond it is inert.  The interval test keeps
//     the binary tree's relative slack (4e-7 >= 6 eps: one subtraction, one rounded reciprocal, one product per plane).
#include "cap_hit_list.h"
#include "cap_kernels.h"
#include "cap_near.h"
#include "cap_query_walk.h"
#include "cap_trace.h"

#include "../../include/capsaicin_hip.h"

namespace cap
{
namespace
{
constexpr double kInstEps   = 5.9604644775390625e-8;  // 2^-24
constexpr double kInstSlack = 32.0;

__device__ __forceinline__ uint32_t inst_float_to_ordered(float f)
{
    const uint32_t u = f2u(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float inst_ordered_to_float(uint32_t o) { return u2f((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// Per instance: W = fl32(inverse(M)), A = inverse(W), kappa, the inert decision, the padded world box and its inflation factor
// (cap_near.h instance_inverse), and what cap_closest_instances prunes with: g <= sigma_min(M) and the world extent Xw (a.near, the
// largest Xw of the table in a.misc[7]; both 0 for an inert instance).
__global__ __launch_bounds__(kBlock) void k_instance_setup(InstanceBuildArgs a)
{
    float    clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t inert = 0;
    float    xw_max = 0.0f;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock)
    {
        const float* d = a.descs + 16 * (size_t)i;
        double       m[12], w[12], wd[12], A[12];
        // the object: an index beyond the table (device indices are not read on the host) makes the instance inert
        const uint32_t    obj  = a.object_index ? a.object_index[i] : 0u;
        bool              live = obj < a.n_objects;
        const InstObject& ob   = a.objects[live ? obj : 0u];
        for (int k = 0; k < 12; ++k) m[k] = (double)d[k], live = live && finite_d(m[k]);
        const uint32_t mask = f2u(d[12]) & 0xFFu;
        float          wf[12];
        double         nA, kappa;
        live = instance_inverse(m, live, w, wf, wd, A, nA, kappa, (float)CAP_INSTANCE_MAX_CONDITION);
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, kf = -1.0f;
        if (live)
        {
            double wlo[3] = {1e308, 1e308, 1e308}, whi[3] = {-1e308, -1e308, -1e308};
            for (int c = 0; c < 8; ++c)
            {
                const double p[3] = {(c & 1) ? ob.bhi[0] : ob.blo[0], (c & 2) ? ob.bhi[1] : ob.blo[1], (c & 4) ? ob.bhi[2] : ob.blo[2]};
                for (int r = 0; r < 3; ++r)
                {
                    const double x = A[4 * r] * p[0] + A[4 * r + 1] * p[1] + A[4 * r + 2] * p[2] + A[4 * r + 3];
                    wlo[r] = fmin(wlo[r], x), whi[r] = fmax(whi[r], x);
                }
            }
            double X = 0.0;
            for (int r = 0; r < 3; ++r) X = fmax(X, fmax(fabs(wlo[r]), fabs(whi[r])));
            const double wt = fmax(fabs(wd[3]), fmax(fabs(wd[7]), fabs(wd[11]))), nW = norm_inf3(wd);
            for (int r = 0; r < 3; ++r)
            {
                // the axis' own share of the error: row r of A (head of this file)
                const double nAr = fabs(A[4 * r]) + fabs(A[4 * r + 1]) + fabs(A[4 * r + 2]);
                const double pad = kInstSlack * kInstEps * (nAr * nW * X + nAr * wt) + 4.0 * kInstEps * X;
                // one ulp outwards of the rounded plane: the stored box contains the padded one
                lo[r] = nextafterf((float)(wlo[r] - pad), -INFINITY), hi[r] = nextafterf((float)(whi[r] + pad), INFINITY);
                live  = live && finite_f(lo[r]) && finite_f(hi[r]);
            }
            kf = (float)(2.0 * kInstSlack * kInstEps * kappa * 1.000001);
        }
        float g = 0.0f, xw = 0.0f;
        if (live) g = near_sigma_min_bound(w), xw = near_world_extent(m, ob.blo, ob.bhi);
        if (!live)
        {
            for (int k = 0; k < 12; ++k) wf[k] = 0.0f;
            for (int r = 0; r < 3; ++r) lo[r] = INFINITY, hi[r] = -INFINITY;
            kf = -1.0f, g = 0.0f, xw = 0.0f;
            ++inert;
        }
        else
            for (int r = 0; r < 3; ++r)
            {
                const float c = (lo[r] + hi[r]) * 0.5f;
                if (finite_f(c)) clo[r] = fminf(clo[r], c), chi[r] = fmaxf(chi[r], c);
            }
        xw_max    = fmaxf(xw_max, xw);
        a.near[i] = make_float2(g, xw);
        a.rec[4 * (size_t)i + 0] = make_float4(wf[0], wf[1], wf[2], wf[3]);
        a.rec[4 * (size_t)i + 1] = make_float4(wf[4], wf[5], wf[6], wf[7]);
        a.rec[4 * (size_t)i + 2] = make_float4(wf[8], wf[9], wf[10], wf[11]);
        a.rec[4 * (size_t)i + 3] = make_float4(u2f(live ? mask : 0u), u2f((uint32_t)ob.root), u2f(obj), 0.f);
        a.box[2 * (size_t)i + 0] = make_float4(lo[0], lo[1], lo[2], kf);
        a.box[2 * (size_t)i + 1] = make_float4(hi[0], hi[1], hi[2], u2f(i));
    }
    // bounds of the live boxes' centres (the Morton grid) and the inert count: one atomic per wave and word
    for (int r = 0; r < 3; ++r)
    {
        float l = clo[r], h = chi[r];
        for (int off = 32; off > 0; off >>= 1) l = fminf(l, __shfl_down(l, off)), h = fmaxf(h, __shfl_down(h, off));
        if ((threadIdx.x & 63u) == 0)
        {
            if (l != INFINITY) atomicMin(&a.misc[r], inst_float_to_ordered(l));
            if (h != -INFINITY) atomicMax(&a.misc[3 + r], inst_float_to_ordered(h));
        }
    }
    for (int off = 32; off > 0; off >>= 1) inert += (uint32_t)__shfl_down((int)inert, off);
    if ((threadIdx.x & 63u) == 0 && inert) atomicAdd(&a.misc[6], inert);
    // (non-negative floats order as their bits)
    for (int off = 32; off > 0; off >>= 1) xw_max = fmaxf(xw_max, __shfl_down(xw_max, off));
    if ((threadIdx.x & 63u) == 0 && xw_max > 0.0f) atomicMax(&a.misc[7], f2u(xw_max));
}

__device__ __forceinline__ uint32_t inst_expand_bits10(uint32_t v)
{
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

// 30-bit Morton code of each live box's centre; inert instances sort behind every live one
__global__ __launch_bounds__(kBlock) void k_instance_morton(InstanceBuildArgs a)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const float4 lo = a.box[2 * (size_t)i], hi = a.box[2 * (size_t)i + 1];
    uint32_t     key = 0xFFFFFFFFu;
    if (lo.w >= 0.0f)
    {
        const float c[3] = {(lo.x + hi.x) * 0.5f, (lo.y + hi.y) * 0.5f, (lo.z + hi.z) * 0.5f};
        uint32_t    q[3];
        // one cell size for the three axes (the largest extent): instances on a plane or a line -- a forest, a street -- are ordered
        // along the axes they spread over, not by the jitter across them
        float ext = 0.0f;
        for (int k = 0; k < 3; ++k) ext = fmaxf(ext, inst_ordered_to_float(a.misc[3 + k]) - inst_ordered_to_float(a.misc[k]));
        for (int k = 0; k < 3; ++k)
        {
            const float n = ext > 0.0f && finite_f(ext) ? (c[k] - inst_ordered_to_float(a.misc[k])) / ext : 0.0f;
            q[k]          = (uint32_t)fminf(fmaxf(n * 1024.0f, 0.0f), 1023.0f);
        }
        key = (inst_expand_bits10(q[0]) << 2) | (inst_expand_bits10(q[1]) << 1) | inst_expand_bits10(q[2]);
    }
    a.keys[0][i] = key;
    a.vals[0][i] = i;
}

__device__ __forceinline__ void tlas_store_empty(float4* e)
{
    e[0] = make_float4(INFINITY, INFINITY, INFINITY, -1.0f);
    e[1] = make_float4(-INFINITY, -INFINITY, -INFINITY, u2f(kInvalidId));
}

// level 0: the instances' box records in sorted order (order == NULL: as they are), padded to an even count
__global__ __launch_bounds__(kBlock) void k_tlas_leaves(const float4* box, const uint32_t* order, uint32_t n, float4* level0)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n + (n & 1u)) return;
    if (j >= n)
    {
        tlas_store_empty(level0 + 2 * (size_t)j);
        return;
    }
    const uint32_t i = order ? order[j] : j;
    level0[2 * (size_t)j] = box[2 * (size_t)i], level0[2 * (size_t)j + 1] = box[2 * (size_t)i + 1];
}

// one level from the one below: entry j = union of entries 2 j and 2 j + 1 (records with k < 0 hold nothing), padded to an even count
__global__ __launch_bounds__(kBlock) void k_tlas_level(const float4* src, uint32_t n_src, float4* dst, uint32_t n_dst)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_dst + (n_dst & 1u)) return;
    if (j >= n_dst)
    {
        tlas_store_empty(dst + 2 * (size_t)j);
        return;
    }
    // (the level below is padded to an even count: entry 2 j + 1 exists)
    const float4 a0 = src[4 * (size_t)j], a1 = src[4 * (size_t)j + 1], b0 = src[4 * (size_t)j + 2], b1 = src[4 * (size_t)j + 3];
    const bool   va = a0.w >= 0.0f, vb = b0.w >= 0.0f && 2 * j + 1 < n_src + (n_src & 1u);
    float4       lo = make_float4(INFINITY, INFINITY, INFINITY, -1.0f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, u2f(kInvalidId));
    if (va) lo = a0, hi = a1;
    if (vb)
    {
        lo = make_float4(fminf(lo.x, b0.x), fminf(lo.y, b0.y), fminf(lo.z, b0.z), fmaxf(lo.w, b0.w));
        hi = make_float4(fmaxf(hi.x, b1.x), fmaxf(hi.y, b1.y), fmaxf(hi.z, b1.z), u2f(kInvalidId));
    }
    hi.w = u2f(kInvalidId);
    dst[2 * (size_t)j] = lo, dst[2 * (size_t)j + 1] = hi;
}

// The top level's box test: `slab` (cap_trace.h) on the box inflated by k |o| (see the head of this file), inclusive at both ends
// like slab, with the relative slack applied to |exit| so that it widens for a negative exit as well.
__device__ __forceinline__ bool tlas_slab(const Ray& r, const float4 lo, const float4 hi, float omax, float tfar, float& tnear_out)
{
    const float g  = lo.w * omax;
    const float ax = ((lo.x - g) - r.o.x) * r.inv.x, bx = ((hi.x + g) - r.o.x) * r.inv.x;
    const float ay = ((lo.y - g) - r.o.y) * r.inv.y, by = ((hi.y + g) - r.o.y) * r.inv.y;
    const float az = ((lo.z - g) - r.o.z) * r.inv.z, bz = ((hi.z + g) - r.o.z) * r.inv.z;
    const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), r.tmin));
    const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tfar));
    tnear_out      = tn;
    return lo.w >= 0.0f && tn <= tf + 4e-7f * fabsf(tf);
}

// ---- the steps the two instanced ray kernels are made of ----
// The bottom level is the binary tree's ray_node_step / ray_pop (cap_query_walk.h) on the object-space ray.
// One top-level node (TopWalk, cap_query_walk.h): tlas_slab on its two children against the caller's far bound, rwb the world ray with
// the caller's lower bound; then down into the nearer one, or their instances into the queue with their entry distances, or up to the
// nearest level that owes a child.
__device__ __forceinline__ TopWalk ray_top_step(const TlasDev& tl, const uint32_t* lds_off, const Ray& rwb, float omax, float tfar, TopWalk t)
{
    const float4* c = tl.tlas + 2 * (size_t)(lds_off[t.level - 1u] + 2u * t.idx);
    const float4  lo0 = c[0], hi0 = c[1], lo1 = c[2], hi1 = c[3];
    float         tn0, tn1;
    const bool    h0 = tlas_slab(rwb, lo0, hi0, omax, tfar, tn0), h1 = tlas_slab(rwb, lo1, hi1, omax, tfar, tn1);
    return top_advance(t, h0, h1, h0 && h1 && tn1 < tn0, f2u(hi0.w), f2u(hi1.w), tn0, tn1);  // the nearer box first
}

// The object-space ray of the contract in instance `inst`: twelve operations, no fused multiply-add.
__device__ __forceinline__ void inst_object_ray(const TlasDev& tl, uint32_t inst, const Ray& rw, v3& o, v3& d)
{
    const float4 w0 = tl.rec[4 * (size_t)inst], w1 = tl.rec[4 * (size_t)inst + 1], w2 = tl.rec[4 * (size_t)inst + 2];
    const v3     r0 = mk3(w0.x, w0.y, w0.z), r1 = mk3(w1.x, w1.y, w1.z), r2 = mk3(w2.x, w2.y, w2.z);
    o = mk3(dot3(r0, rw.o) + w0.w, dot3(r1, rw.o) + w1.w, dot3(r2, rw.o) + w2.w);
    d = mk3(dot3(r0, rw.d), dot3(r1, rw.d), dot3(r2, rw.d));
}

// Entering the instance at the head of the queue, whose box the ray enters at tn: only if tn still passes against the caller's far
// bound as it is now (the comparison tlas_slab made, with the bound the nearer instance left), the mask lets the instance in (desc.mask
// & inclusion; the mesh byte joins it per triangle; 0 for an inert one) and the object-space ray is one the walk traces.  The root of
// the object's tree rides in the record's mask word.  The results go through references into the kernel's own variables.
__device__ __forceinline__ bool ray_enter_instance(const TlasDev& tl, uint32_t mask, uint32_t inst, float tn, float tfar, const Ray& rw, uint32_t& imask,
                                                   Ray& r, int& root)
{
    if (!(tn <= tfar + 4e-7f * fabsf(tfar))) return false;
    const float4 w3 = tl.rec[4 * (size_t)inst + 3];
    imask           = f2u(w3.x) & mask;
    if (imask == 0u) return false;
    v3 o, d;
    inst_object_ray(tl, inst, rw, o, d);
    if (!query_ray_ok(make_float4(o.x, o.y, o.z, rw.tmin), make_float4(d.x, d.y, d.z, rw.tmax))) return false;
    r    = make_ray(o, d, rw.tmin, rw.tmax);
    root = (int)f2u(w3.y);
    return true;
}

// Closest (MODE 0) / first accepted (1) / occlusion (2) over the instances, one ray per lane.
// Top level: no stack.  The tree is implicit, so a node is (level, index), its sibling index ^ 1 and its ancestors index >> levels;
// `pending` holds one bit per level, set where the walk went to the nearer of two children that both passed and still owes the other.
// Bottom level: k_query_binary_f's walk of the object's binary tree (ray_node_step / ray_pop) on the object-space ray of the contract,
// with the shared best_t; the lane's LDS slice is that walk's stack alone.  The tree's root rides in the instance record's mask word
// (w3.y): the scene's root in the scene's pools, or the object's in the forest's (bvh.nodes / bvh.tris point at either; bvh.root is
// not read).
// One loop, three kinds of step -- a top-level node (ray_top_step), entering an instance (ray_enter_instance: the ray transform, 12
// multiply-adds and make_ray's divisions), a bottom-level node or leaf -- so that the lanes of a wave that are at the top level
// advance while others are inside an instance.
// The two instances under a level-1 node wait in (todo0, todo1), the nearer box first; each is entered only if its entry distance
// still passes against best_t as it is then (the comparison tlas_slab made, with the bound the nearer instance left).
constexpr int inst_blocks(int STACK) { return STACK <= 24 ? 6 : STACK <= 32 ? 4 : 2; }

template <int STACK, int MODE>
__global__ __launch_bounds__(kBlock, inst_blocks(STACK)) void k_query_inst(BvhDev bvh, QueryArgs q, TlasDev tl, RayFilter f, uint32_t* inst_out)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    __shared__ uint32_t lds_off[kTlasMaxLevels + 1];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    if (threadIdx.x <= tl.top) lds_off[threadIdx.x] = tl.level_off[threadIdx.x];
    __syncthreads();
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < q.n; j += gridDim.x * kBlock)
    {
        const float4 a = q.rays[2 * (size_t)j], b = q.rays[2 * (size_t)j + 1];
        const Ray    rw   = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
        const float  omax = fmaxf(fabsf(a.x), fmaxf(fabsf(a.y), fabsf(a.z)));
        float        best_t = b.w, best_u = 0.f, best_v = 0.f;
        uint32_t     best_gid = kInvalidId, best_inst = kInvalidId;
        bool         found = false;  // MODE 1, 2: the query is over
        TopWalk      top = top_start(tl);
        // bottom level
        bool     in_blas = false;
        Ray      r       = rw;
        uint32_t inst = 0u, imask = 0u;
        int      node = 0, sp = 0;
        bool     walk = query_ray_ok(a, b) && bvh.tri_count != 0u;
        while (walk)
        {
            if (in_blas)
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
                        if (f.tri_mask && (f.tri_mask[gid] & imask) == 0u) continue;
                        if (MODE != 0)
                            best_t = t, best_u = u, best_v = v, best_gid = gid, best_inst = inst, found = true;
                        else if (t < best_t || (t == best_t && (inst < best_inst || (inst == best_inst && gid < best_gid))))
                            best_t = t, best_u = u, best_v = v, best_gid = gid, best_inst = inst;
                    }
                    if (found) break;
                }
                in_blas = ray_pop(stack, sp, node);
                continue;
            }
            if (top.todo0 != kInvalidId)
            {
                inst           = top.todo0;
                const float tn = top.todo0_d;
                top            = top_pop(top);
                if (ray_enter_instance(tl, f.mask, inst, tn, best_t, rw, imask, r, node)) sp = 0, in_blas = true;
                continue;
            }
            if (top.done) break;
            top = ray_top_step(tl, lds_off, rw, omax, best_t, top);
        }
        if (MODE == 2)
            static_cast<uint32_t*>(q.out)[j] = found ? 1u : 0u;
        else
        {
            static_cast<float4*>(q.out)[j] = make_float4(best_t, best_u, best_v, u2f(best_gid));
            if (inst_out) inst_out[j] = best_inst;
        }
    }
}

// ---- multi-hit over the instances (cap_trace_instances_multi) ----
// A ray's first k pairs in (t, instance, triangle) order, the number of its pairs, or both, in cap_hit_list.h's InstHitList: HitList with
// the instance between t and the triangle.

// Workgroups per CU: the LDS slice allows inst_blocks(STACK); the list's 3 K registers (and cursor, count, the second lower bound) take
// it down to the most that leave every instantiation without scratch (tools/kernel_regs.sh; the table is in DESIGN.md): six (80
// VGPRs) at K = 1, four (128) at K = 4 -- five (96) spill --, three (168) at K = 8 -- four spill -- and two (256) at K = 16.
constexpr int inst_multi_blocks(int STACK, int K)
{
    const int by_regs = K <= 1 ? 6 : K <= 4 ? 4 : K <= 8 ? 3 : 2;
    return inst_blocks(STACK) < by_regs ? inst_blocks(STACK) : by_regs;
}

// k_query_inst's closest-mode loop with the list in place of the best record.  The pruning bound `tfar` -- slot K - 1's t, or tmax
// while counting -- stands wherever best_t stands there: the bottom-level slab, tlas_slab and the `still` re-check of a queued
// instance.  All three are inclusive (tn <= tf (1 + slack), tf = min(exit, tfar)), so an instance or box entered exactly at the k-th
// t is still opened and an equal-t pair with a lower (instance, triangle) still displaces the k-th entry: the list is exact whatever
// the visiting order.  Paging: only pairs above the cursor (t_c, i_c, g_c) -- slot k - 1 of the ray's two pages -- are offered; pairs
// below t_c lie outside every later page, so the BOX tests take lo = max(tmin, t_c) as their lower bound (inclusive too: a pair at
// t_c with a higher (instance, triangle) is kept), while the triangle test keeps the ray's own tmin and with it its bits.
// Write-out as query.hip's multi_write: (u, v) are not kept in the list; each listed pair is tested again, on the object-space ray
// rebuilt from its instance record and the triangle's record in bvh.tris_by_id.  That record equals the one the walk read in its
// first twelve words (the scene's and the forest's are written by the same triangle setup from the same vertices; only word 12, the
// id, is renumbered by k_forest_relocate), and the ray is rebuilt by the same operations, so (t, u, v) are the traversal's.
template <int STACK, int K, bool COUNT>
__global__ __launch_bounds__(kBlock, inst_multi_blocks(STACK, K)) void k_query_inst_multi(BvhDev bvh, MultiArgs m, TlasDev tl, RayFilter f, uint32_t* inst_out)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    __shared__ uint32_t lds_off[kTlasMaxLevels + 1];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    if (threadIdx.x <= tl.top) lds_off[threadIdx.x] = tl.level_off[threadIdx.x];
    __syncthreads();
    const QueryArgs& q = m.q;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < q.n; j += gridDim.x * kBlock)
    {
        const float4 a = q.rays[2 * (size_t)j], b = q.rays[2 * (size_t)j + 1];
        const Ray    rw   = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
        const float  omax = fmaxf(fabsf(a.x), fmaxf(fabsf(a.y), fabsf(a.z)));
        float4* const   page  = static_cast<float4*>(q.out) + (size_t)j * m.k;
        uint32_t* const ipage = inst_out + (size_t)j * m.k;
        InstHitList<K>  L;
        L.init(m.k, rw.tmax);
        // the cursor: slot k - 1 of both pages when paging, else (-inf, 0, 0), below every pair
        float    tc = -__builtin_inff();
        uint32_t ic = 0u, gc = 0u, count = 0u;
        if (m.resume)
        {
            const float4 e = page[m.k - 1u];
            tc = e.x, gc = f2u(e.w), ic = ipage[m.k - 1u];
        }
        const float lo  = fmaxf(rw.tmin, tc);  // the box tests' lower bound
        Ray         rwb = rw;
        rwb.tmin        = lo;
        TopWalk     top = top_start(tl);
        // bottom level: r for the triangles, rb (its tmin = lo) for the boxes
        bool     in_blas = false;
        Ray      r = rw, rb = rwb;
        uint32_t inst = 0u, imask = 0u;
        int      node = 0, sp = 0;
        bool     walk = query_ray_ok(a, b) && bvh.tri_count != 0u;
        while (walk)
        {
            const float tfar = COUNT ? rw.tmax : L.t[K - 1];
            if (in_blas)
            {
                if (node >= 0)
                {
                    if (ray_node_step<STACK>(bvh, rb, tfar, stack, node, sp)) continue;
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
                        if (f.tri_mask && (f.tri_mask[gid] & imask) == 0u) continue;
                        // multi_offer's rule with the instance between t and the triangle
                        if (InstHitList<K>::before(tc, ic, gc, t, inst, gid))
                        {
                            if (COUNT) ++count;
                            if (L.admits(t, inst, gid)) L.insert(t, inst, gid);
                        }
                    }
                }
                in_blas = ray_pop(stack, sp, node);
                continue;
            }
            if (top.todo0 != kInvalidId)
            {
                inst           = top.todo0;
                const float tn = top.todo0_d;
                top            = top_pop(top);
                if (ray_enter_instance(tl, f.mask, inst, tn, tfar, rw, imask, r, node)) rb = r, rb.tmin = lo, sp = 0, in_blas = true;
                continue;
            }
            if (top.done) break;
            top = ray_top_step(tl, lds_off, rwb, omax, tfar, top);
        }
        if (COUNT) m.counts[j] = count;
        const int skip = K - (int)m.k;  // the placeholders
        uint32_t  cur  = kInvalidId;    // the instance r holds the object-space ray of: consecutive listed pairs often share one
#pragma unroll
        for (int s = 0; s < K; ++s)
            if (s >= skip)
            {
                float u = 0.f, v = 0.f;
                if (L.g[s] != kInvalidId)
                {
                    if (L.i[s] != cur)
                    {
                        v3 o, d;
                        inst_object_ray(tl, L.i[s], rw, o, d);
                        r   = make_ray(o, d, rw.tmin, rw.tmax);
                        cur = L.i[s];
                    }
                    const float4* rec = bvh.tris_by_id + 4 * (size_t)L.g[s];
                    float         t;
                    tri_test(r, rec[0], rec[1], rec[2], t, u, v);
                }
                page[s - skip]  = make_float4(L.t[s], u, v, u2f(L.g[s]));
                ipage[s - skip] = L.i[s];
            }
    }
}

// An object's tree, built by the scene's builders on the object's triangles alone (local node, record and triangle numbers), made part
// of the forest in place: node and record numbers of the pools, the scene's triangle ids.
__global__ __launch_bounds__(kBlock) void k_forest_relocate(ForestRelocArgs a)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_tris) return;
    float4 id = a.tris[4 * (size_t)i + 3];
    id.x      = u2f(f2u(id.x) + a.first_triangle);
    a.tris[4 * (size_t)i + 3] = id;
    if (i + 1u >= a.n_tris) return;
    const float4 q3 = a.nodes[4 * (size_t)i + 3];
    uint32_t     link[4] = {f2u(q3.x), f2u(q3.y), f2u(q3.z), f2u(q3.w)};
    for (int k = 0; k < 4; ++k)
    {
        if ((int)link[k] >= 0)
            link[k] += a.node_base;  // an inner node
        else if (k < 2)
            link[k] = ~(~link[k] + a.rec_base);  // the binary tree's leaf: ~record
        else
        {
            const uint32_t code = ~link[k];  // the walk's leaf: ~(first | (count - 1) << kLeafCountShift)
            link[k]             = ~(((code & kLeafFirstMask) + a.rec_base) | (code & ~kLeafFirstMask));
        }
    }
    a.nodes[4 * (size_t)i + 3] = make_float4(u2f(link[0]), u2f(link[1]), u2f(link[2]), u2f(link[3]));
}
}  // namespace

uint32_t tlas_layout(uint32_t n, uint32_t level_off[kTlasMaxLevels], uint32_t* total)
{
    uint32_t level = 0, off = 0, cnt = n;
    while (true)
    {
        level_off[level] = off;
        off += cnt + (cnt & 1u);
        if (cnt <= 1u) break;
        cnt = (cnt + 1u) / 2u;
        ++level;
    }
    if (total) *total = off;
    return level;
}

void launch_instances_build(hipStream_t stream, const InstanceBuildArgs& a)
{
    const uint32_t n = a.n;
    if (n == 0) return;
    const uint32_t blocks = (n + kBlock - 1) / kBlock;
    // bounds = (+inf x 3, -inf x 3) in the ordered encoding, inert count 0
    const uint32_t init[8] = {0xFF800000u, 0xFF800000u, 0xFF800000u, 0x007FFFFFu, 0x007FFFFFu, 0x007FFFFFu, 0u, 0u};
    (void)hipMemcpyAsync(a.misc, init, sizeof(init), hipMemcpyHostToDevice, stream);
    hipLaunchKernelGGL(k_instance_setup, dim3(blocks < 1024u ? blocks : 1024u), dim3(kBlock), 0, stream, a);
    const uint32_t* order = nullptr;
    if (n > 2)  // (one or two instances are the two children of the walk's first step in any order)
    {
        hipLaunchKernelGGL(k_instance_morton, dim3(blocks), dim3(kBlock), 0, stream, a);
        order = a.vals[launch_radix_sort_pairs(stream, a.keys, a.vals, n, a.hist, a.scan)];
    }
    uint32_t       off[kTlasMaxLevels];
    const uint32_t top = tlas_layout(n, off, nullptr);
    hipLaunchKernelGGL(k_tlas_leaves, dim3((n + 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a.box, order, n, a.tlas);
    uint32_t cnt = n;
    for (uint32_t l = 1; l <= top; ++l)
    {
        const uint32_t next = (cnt + 1u) / 2u;
        hipLaunchKernelGGL(k_tlas_level, dim3((next + 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a.tlas + 2 * (size_t)off[l - 1], cnt,
                           a.tlas + 2 * (size_t)off[l], next);
        cnt = next;
    }
}

void launch_forest_relocate(hipStream_t stream, const ForestRelocArgs& a)
{
    if (a.n_tris) hipLaunchKernelGGL(k_forest_relocate, dim3((a.n_tris + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
}

void launch_query_instances(const LaunchCfg& cfg, const BvhDev& bvh, const QueryArgs& q, const TlasDev& tl, const RayFilter& f, int mode, uint32_t* inst_out,
                            uint32_t depth)
{
    with_instance_stack(cfg, depth, [&](auto S) {
        constexpr int s = decltype(S)::value;
        if (mode == 2)
            launch_lanes<k_query_inst<s, 2>>(cfg, q.n, false, bvh, q, tl, f, (uint32_t*)nullptr);
        else if (mode == 1)
            launch_lanes<k_query_inst<s, 1>>(cfg, q.n, false, bvh, q, tl, f, inst_out);
        else
            launch_lanes<k_query_inst<s, 0>>(cfg, q.n, false, bvh, q, tl, f, inst_out);
    });
}

void launch_query_instances_multi(const LaunchCfg& cfg, const BvhDev& bvh, const MultiArgs& m, const TlasDev& tl, const RayFilter& f, uint32_t* inst_out,
                                  uint32_t depth)
{
    with_instance_stack(cfg, depth, [&](auto S) {
        with_k_bucket(m.k, [&](auto K) {
            with_flag(m.counts != nullptr, [&](auto COUNT) {
                launch_lanes<k_query_inst_multi<decltype(S)::value, decltype(K)::value, decltype(COUNT)::value>>(cfg, m.q.n, false, bvh, m, tl, f, inst_out);
            });
        });
    });
}
}  // namespace cap
