// refit.hip — in-place refit of the trees of the last cap_bvh_build to moved vertices (cap_bvh_refit; DXR PERFORM_UPDATE).
//
// The topology stays: the binary tree's nodes and leaf order, the 8-wide view's child_base / tri_base / imask / tvalid and slot
// assignment, both leaf orders of the intersection records.  Only what the build derives from the vertices is recomputed, with the
// build's own arithmetic: triangle setup (bvh.hip k_tri_setup), the binary boxes by the build's climb (bvh.hip k_refit) over parent
// links derived from the nodes, the wide planes bottom-up through the collapse's quantiser (cap_wide_quant.h).  With unchanged
// positions the trees come out byte for byte as the build left them (one exception: where the device SAH build halved a segment by
// position it stored the segment's box for both children, ploc.hip k_sah_split; the climb leaves each child's own union); with moved
// ones the hits are those of a fresh build of the moved scene (the hit rule never looks at boxes; DESIGN.md "Intersection contract").
//
// One stream, no host round trip inside: the caller reads the scene bounds once (the wide padding depends on them) and syncs once.
#include "cap_kernels.h"
#include "cap_wide.h"
#include "cap_wide_quant.h"

namespace cap
{
namespace
{
constexpr uint32_t kVisitsBlocks = 1024;  // partial sums of the tree metric: a fixed grid, so the sum is the same on every run

// parent links of the kept binary tree from its nodes (the device builders' parent array is sort scratch, the host SAH build never
// writes one): (node << 1) | slot, internal nodes first, then the leaves; the root (node 0) has none
__global__ __launch_bounds__(kBlock) void k_refit_links(const float4* nodes, uint32_t n, uint32_t* parent)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i + 1u >= n) return;
    const float4 q = nodes[4 * (size_t)i + 3];
    const int    c[2] = {(int)f2u(q.x), (int)f2u(q.y)};
    for (uint32_t s = 0; s < 2u; ++s)
        parent[c[s] >= 0 ? (size_t)c[s] : (size_t)(n - 1u) + (size_t)~c[s]] = (i << 1) | s;
    if (i == 0) parent[0] = 0xffffffffu;
}

__device__ __forceinline__ double half_area(float lx, float ly, float lz, float hx, float hy, float hz)
{
    const double dx = (double)hx - (double)lx, dy = (double)hy - (double)ly, dz = (double)hz - (double)lz;
    return dx * dy + dy * dz + dz * dx;
}

// expected node visits of the binary tree, first half: per workgroup the sum of the inner children's box areas
__global__ __launch_bounds__(kBlock) void k_tree_visits_partial(const float4* nodes, uint32_t n_nodes, double* partial)
{
    __shared__ double s_wave[kBlock / 64];
    double            sum = 0.0;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n_nodes; i += gridDim.x * kBlock)
    {
        const float4 a = nodes[4 * (size_t)i], b = nodes[4 * (size_t)i + 1], c = nodes[4 * (size_t)i + 2], d = nodes[4 * (size_t)i + 3];
        if ((int)f2u(d.x) >= 0) sum += half_area(a.x, a.y, a.z, a.w, b.x, b.y);
        if ((int)f2u(d.y) >= 0) sum += half_area(b.z, b.w, c.x, c.y, c.z, c.w);
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double t = 0.0;
        for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_wave[w];
        partial[blockIdx.x] = t;
    }
}
// second half, one wave: 1 + sum / (root box area)
__global__ __launch_bounds__(64) void k_tree_visits_final(const float4* nodes, const double* partial, uint32_t n_partial, double* out)
{
    double sum = 0.0;
    for (uint32_t b = threadIdx.x; b < n_partial; b += 64u) sum += partial[b];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if (threadIdx.x == 0)
    {
        const float4 a = nodes[0], b = nodes[1], c = nodes[2];
        const double root = half_area(fminf(a.x, b.z), fminf(a.y, b.w), fminf(a.z, c.x), fmaxf(a.w, c.y), fmaxf(b.x, c.z), fmaxf(b.y, c.w));
        out[0] = 1.0 + sum / root;
    }
}

// a triangle's box as the binary tree holds it: the leaf padding of bvh.hip k_refit (and of every other builder)
__device__ __forceinline__ void padded_triangle_box(const float4* tri_box, uint32_t g, float lo[3], float hi[3])
{
    const float4 l = tri_box[2 * (size_t)g], h = tri_box[2 * (size_t)g + 1];
    lo[0] = l.x, lo[1] = l.y, lo[2] = l.z, hi[0] = h.x, hi[1] = h.y, hi[2] = h.z;
    for (int k = 0; k < 3; ++k)
    {
        const float pad = 1e-5f * fmaxf(1.0f, fmaxf(fabsf(lo[k]), fabsf(hi[k])));
        lo[k] -= pad, hi[k] += pad;
    }
}

// One level of the 8-wide view, one thread per node (deeper levels done): every child's float box -- an inner child's from the
// scratch its own refit left, a leaf child's as the union of its records' padded triangle boxes -- is the box the collapse read
// from the binary node; then the collapse's padding, node box, grid and planes.  Words 4..6 (topology) stay as they are.
__global__ __launch_bounds__(kBlock) void k_wide_refit(WideRefitArgs a)
{
    const uint32_t w = a.begin + blockIdx.x * kBlock + threadIdx.x;
    if (w >= a.end) return;
    uint4*   node = reinterpret_cast<uint4*>(a.nodes8 + (size_t)w * kWideNodeStride);
    uint32_t word[kWideNodeWords];
    for (uint32_t k = 0; k < kWideNodeWords / 4u; ++k)
    {
        const uint4 v = node[k];
        word[4 * k] = v.x, word[4 * k + 1] = v.y, word[4 * k + 2] = v.z, word[4 * k + 3] = v.w;
    }
    const uint32_t child_base = word[4], tri_base = word[5], tvalid = word[6] & 0xffffffu, imask = word[6] >> 24;
    float          flo[8][3], fhi[8][3], nflo[3] = {INFINITY, INFINITY, INFINITY}, nfhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t       used = 0u;
    for (uint32_t s = 0; s < 8u; ++s)
    {
        for (int k = 0; k < 3; ++k) flo[s][k] = INFINITY, fhi[s][k] = -INFINITY;
        if (imask & (1u << s))
        {
            const float* b = a.boxes + 6 * (size_t)(child_base + (uint32_t)__popc(imask & ((1u << s) - 1u)));
            for (int k = 0; k < 3; ++k) flo[s][k] = b[k], fhi[s][k] = b[3 + k];
        }
        else if (tvalid & (0x010101u << s))
        {
            for (uint32_t j = 0; j < kWideLeafMax; ++j)
            {
                const uint32_t bit = j * 8u + s;
                if (!(tvalid & (1u << bit))) continue;
                const uint32_t r = tri_base + (uint32_t)__popc(tvalid & ((1u << bit) - 1u));
                const uint32_t g = f2u(a.tris8[4 * (size_t)r + 3].x);  // the record's word 12: its global triangle id
                float          lo[3], hi[3];
                padded_triangle_box(a.tri_box, g, lo, hi);
                for (int k = 0; k < 3; ++k) flo[s][k] = fminf(flo[s][k], lo[k]), fhi[s][k] = fmaxf(fhi[s][k], hi[k]);
            }
        }
        else
            continue;
        used |= 1u << s;
        for (int k = 0; k < 3; ++k) nflo[k] = fminf(nflo[k], flo[s][k]), nfhi[k] = fmaxf(nfhi[k], fhi[s][k]);
    }
    float* out_box = a.boxes + 6 * (size_t)w;
    for (int k = 0; k < 3; ++k) out_box[k] = nflo[k], out_box[3 + k] = nfhi[k];
    // the collapse's padded child boxes (double) and node box
    double clo[3], chi[3], nlo[3] = {1e300, 1e300, 1e300}, nhi[3] = {-1e300, -1e300, -1e300};
    auto   child = [&](uint32_t s) {
        for (int k = 0; k < 3; ++k)
        {
            if (a.one_triangle)
            {
                // the one-triangle scene's only child: the scene bounds padded in double (wide_builder.cpp build_wide_tree)
                const float4 l = a.tri_box[0], h = a.tri_box[1];
                const double lo = k == 0 ? l.x : (k == 1 ? l.y : l.z), hi = k == 0 ? h.x : (k == 1 ? h.y : h.z);
                const double rp = 1e-5 * fmax(1.0, fmax(fabs(lo), fabs(hi)));
                clo[k] = (lo - rp) - a.pad, chi[k] = (hi + rp) + a.pad;
            }
            else
                clo[k] = (double)flo[s][k] - a.pad, chi[k] = (double)fhi[s][k] + a.pad;
        }
    };
    for (uint32_t s = 0; s < 8u; ++s)
        if (used & (1u << s))
        {
            child(s);
            for (int k = 0; k < 3; ++k) nlo[k] = fmin(nlo[k], clo[k]), nhi[k] = fmax(nhi[k], chi[k]);
        }
    word[0] = word[1] = word[2] = word[3] = word[7] = 0u;
    for (uint32_t k = 8; k < kWideNodeWords; ++k) word[k] = 0u;
    const WideGrid grid = wide_grid(nlo, nhi, word);
    for (uint32_t s = 0; s < 8u; ++s)
        if (used & (1u << s))
        {
            child(s);
            wide_quantise(grid, clo, chi, (int)s, word);
        }
    for (uint32_t k = 0; k < kWideNodeWords / 4u; ++k) node[k] = make_uint4(word[4 * k], word[4 * k + 1], word[4 * k + 2], word[4 * k + 3]);
}
}  // namespace

void launch_refit_binary(hipStream_t stream, const BvhBuildArgs& a)
{
    const uint32_t n = a.tri_count;
    if (n == 0) return;
    launch_bvh_setup(stream, a);  // bounds reset, arrival counters cleared, k_tri_setup
    if (n >= 2) hipLaunchKernelGGL(k_refit_links, dim3((n - 1u + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a.nodes, n, a.parent);
    launch_bvh_refit_climb(stream, a);
}

size_t tree_visits_scratch() { return kVisitsBlocks; }

void launch_tree_visits(hipStream_t stream, const float4* nodes, uint32_t n_tris, double* scratch, double* out)
{
    if (n_tris < 2) return;
    const uint32_t nn = n_tris - 1u, blocks = std::min<uint32_t>(kVisitsBlocks, (nn + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_tree_visits_partial, dim3(blocks), dim3(kBlock), 0, stream, nodes, nn, scratch);
    hipLaunchKernelGGL(k_tree_visits_final, dim3(1), dim3(64), 0, stream, nodes, scratch, blocks, out);
}

void launch_refit_wide(hipStream_t stream, WideRefitArgs a, const std::vector<uint32_t>& level_begin)
{
    for (size_t l = level_begin.size(); l-- > 1;)
    {
        a.begin = level_begin[l - 1], a.end = level_begin[l];
        if (a.end > a.begin) hipLaunchKernelGGL(k_wide_refit, dim3((a.end - a.begin + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
    }
}
}  // namespace cap
