// pseudonormal.hip — the angle-weighted pseudonormal table behind cap_signed_distance (Baerentzen & Aanaes 2005), built on the device
// from the scene's ORIGINAL vertices (positions / indices / tri_ids / mesh_offsets as bvh.hip's k_tri_setup reads them), gfx950.
// include/capsaicin_hip.h ("signed distance") has the definition; DESIGN.md "Signed distance" the reasons.
//
// Pipeline (one stream, no host round trip; C = 3 x triangles corners = half-edges):
//   k_pn_setup        per triangle: liveness, the face normal Nf and the three corner angles in binary64, the corners' position keys
//   corner sort       three stable radix sorts (launch_radix_sort_pairs) over the z, y and x bits: equal positions become runs, and
//                     inside a run the corners stay in ascending (triangle, corner) order
//   k_pn_heads, scan, k_pn_weld      a flag where a run starts, an exclusive scan, the weld id of every corner
//   k_pn_vertex_sums  the first corner of a run adds angle x Nf along the run, in that order, and stores the sum for every corner of it
//   k_pn_halfedges    (lower, higher) weld id of each half-edge
//   edge sort         two stable radix sorts, over the higher and then the lower id
//   k_pn_edge_sums    the first half-edge of a run adds Nf along the run, classifies the edge, and stores the sum for every member
// A run is summed by ONE thread from its first element on: the order of the additions is the order of the contract whatever the
// valence, at the price of a thread that works alone on a vertex of valence 10^6.  A degenerate triangle's corners carry the key
// kPnDead (a NaN pattern no live corner has: every coordinate of a live triangle is finite), sort behind everything and are skipped.
#include "cap_kernels.h"

namespace cap
{
namespace
{
constexpr uint32_t kPnDead = 0xFFFFFFFFu;

// the coordinate with -0 mapped to +0: what is welded and what every sum is made of
__device__ __forceinline__ float pn_canon(float x) { return x + 0.0f; }

struct d3
{
    double x, y, z;
};
__device__ __forceinline__ d3     dsub(const d3 a, const d3 b) { return d3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ d3     dcross(const d3 a, const d3 b) { return d3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double ddot(const d3 a, const d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double dangle(const d3 a, const d3 b)
{
    const d3 c = dcross(a, b);
    return atan2(sqrt(ddot(c, c)), ddot(a, b));
}

__global__ __launch_bounds__(kBlock) void k_pn_setup(PseudonormalArgs a)
{
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= a.tri_count) return;
    const uint4    id = a.tri_ids[g];
    const uint4    mo = a.mesh_offsets[id.x];
    const uint32_t io = mo.y + 3u * id.y;
    float          p[3][3];
    bool           finite = true;
    for (int k = 0; k < 3; ++k)
    {
        const uint32_t v = mo.x + a.indices[io + k];
        for (int j = 0; j < 3; ++j)
        {
            p[k][j] = pn_canon(a.positions[3 * (size_t)v + j]);
            finite  = finite && fabsf(p[k][j]) < __builtin_inff();  // (a NaN fails the comparison)
        }
    }
    const d3 v0{p[0][0], p[0][1], p[0][2]}, v1{p[1][0], p[1][1], p[1][2]}, v2{p[2][0], p[2][1], p[2][2]};
    const d3 e01 = dsub(v1, v0), e02 = dsub(v2, v0), e12 = dsub(v2, v1);
    const d3 n = dcross(e01, e02);
    // (two corners at one position give a zero cross product: the weld ids need not be known here)
    const bool   live = finite && !(n.x == 0.0 && n.y == 0.0 && n.z == 0.0);
    const size_t c    = 3 * (size_t)g;
    if (!live)
    {
        for (int k = 0; k < 3; ++k) a.kx[c + k] = a.ky[c + k] = a.kz[c + k] = kPnDead;
        for (int k = 0; k < 3; ++k) a.nf[c + k] = a.ang[c + k] = 0.0;
        atomicAdd(&a.stats[5], 1u);
        return;
    }
    const double len = sqrt(ddot(n, n));
    const d3     nf{n.x / len, n.y / len, n.z / len};
    a.nf[c] = nf.x, a.nf[c + 1] = nf.y, a.nf[c + 2] = nf.z;
    const d3 zero{0.0, 0.0, 0.0};
    a.ang[c]     = dangle(e01, e02);
    a.ang[c + 1] = dangle(e12, dsub(zero, e01));
    a.ang[c + 2] = dangle(dsub(zero, e02), dsub(zero, e12));
    for (int k = 0; k < 3; ++k) a.kx[c + k] = f2u(p[k][0]), a.ky[c + k] = f2u(p[k][1]), a.kz[c + k] = f2u(p[k][2]);
    float* const t = a.table + 21 * (size_t)g;
    t[0] = (float)nf.x, t[1] = (float)nf.y, t[2] = (float)nf.z;
}

__global__ __launch_bounds__(kBlock) void k_pn_pairs(const uint32_t* src, uint32_t* keys, uint32_t* vals, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) keys[i] = src[i], vals[i] = i;
}
__global__ __launch_bounds__(kBlock) void k_pn_gather(const uint32_t* src, const uint32_t* vals, uint32_t* keys, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) keys[i] = src[vals[i]];
}

// sorted position i starts a run: its element's three key words differ from its predecessor's
__device__ __forceinline__ bool pn_head(const uint32_t* perm, const uint32_t* k0, const uint32_t* k1, const uint32_t* k2, uint32_t i)
{
    if (i == 0u) return true;
    const uint32_t c = perm[i], b = perm[i - 1u];
    return k0[c] != k0[b] || k1[c] != k1[b] || (k2 && k2[c] != k2[b]);
}

__global__ __launch_bounds__(kBlock) void k_pn_heads(PseudonormalArgs a, const uint32_t* perm, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) a.flag[i] = pn_head(perm, a.kx, a.ky, a.kz, i) ? 1u : 0u;
}
// a.flag holds the exclusive scan of the heads
__global__ __launch_bounds__(kBlock) void k_pn_weld(PseudonormalArgs a, const uint32_t* perm, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) a.weld[perm[i]] = a.flag[i] + (pn_head(perm, a.kx, a.ky, a.kz, i) ? 1u : 0u) - 1u;
}

// adds the set lanes of `yes` into *counter with one atomic per wave; every lane of the wave must arrive
__device__ __forceinline__ void pn_count(bool yes, uint32_t* counter)
{
    const unsigned long long m = __ballot(yes);
    if (m != 0ull && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(m)) atomicAdd(counter, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(kBlock) void k_pn_vertex_sums(PseudonormalArgs a, const uint32_t* perm, uint32_t n)
{
    const uint32_t i    = blockIdx.x * kBlock + threadIdx.x;
    bool           head = false;
    if (i < n)
    {
        const uint32_t c = perm[i];
        head             = a.kx[c] != kPnDead && (i == 0u || a.weld[perm[i - 1u]] != a.weld[c]);
        if (head)
        {
            const uint32_t w  = a.weld[c];
            double         sx = 0.0, sy = 0.0, sz = 0.0;
            uint32_t       j = i;
            for (; j < n && a.weld[perm[j]] == w; ++j)
            {
                const uint32_t q  = perm[j];
                const double   an = a.ang[q];
                const double*  nf = a.nf + 3 * (size_t)(q / 3u);
                sx += an * nf[0], sy += an * nf[1], sz += an * nf[2];
            }
            const float fx = (float)sx, fy = (float)sy, fz = (float)sz;
            for (uint32_t k = i; k < j; ++k)
            {
                const uint32_t q = perm[k];
                float* const   t = a.table + 21 * (size_t)(q / 3u) + 3u * (4u + q % 3u);
                t[0] = fx, t[1] = fy, t[2] = fz;
            }
        }
    }
    pn_count(head, &a.stats[0]);
}

// half-edge h = 3 g + k runs from corner k to corner (k + 1) % 3 of triangle g: CAP_FEATURE_EDGE_V0V1 + k.  (lower, higher) weld id
// into (ky, kz): the corner sort is done with them, kx still marks the dead.
__global__ __launch_bounds__(kBlock) void k_pn_halfedges(PseudonormalArgs a, uint32_t n)
{
    const uint32_t h = blockIdx.x * kBlock + threadIdx.x;
    if (h >= n) return;
    if (a.kx[h] == kPnDead)
    {
        a.ky[h] = a.kz[h] = kPnDead;  // (a weld id is below C <= 2^32 - 1)
        return;
    }
    const uint32_t g = h / 3u, k = h % 3u;
    const uint32_t w0 = a.weld[h], w1 = a.weld[3u * g + (k + 1u) % 3u];
    a.ky[h] = w0 < w1 ? w0 : w1, a.kz[h] = w0 < w1 ? w1 : w0;
}

__global__ __launch_bounds__(kBlock) void k_pn_edge_sums(PseudonormalArgs a, const uint32_t* perm, uint32_t n)
{
    const uint32_t i    = blockIdx.x * kBlock + threadIdx.x;
    bool           head = false, boundary = false, nonmanifold = false, inconsistent = false;
    if (i < n)
    {
        const uint32_t h0 = perm[i];
        head              = a.kx[h0] != kPnDead && pn_head(perm, a.ky, a.kz, nullptr, i);
        if (head)
        {
            const uint32_t lo = a.ky[h0], hi = a.kz[h0];
            double         sx = 0.0, sy = 0.0, sz = 0.0;
            uint32_t       j = i, forward = 0u;  // forward: members that run from the lower to the higher weld id
            for (; j < n; ++j)
            {
                const uint32_t h = perm[j];
                if (a.ky[h] != lo || a.kz[h] != hi) break;
                const double* nf = a.nf + 3 * (size_t)(h / 3u);
                sx += nf[0], sy += nf[1], sz += nf[2];
                forward += a.weld[h] == lo ? 1u : 0u;
            }
            const uint32_t m = j - i;
            boundary = m == 1u, nonmanifold = m > 2u, inconsistent = m == 2u && forward != 1u;
            const float fx = (float)sx, fy = (float)sy, fz = (float)sz;
            for (uint32_t k = i; k < j; ++k)
            {
                const uint32_t h = perm[k];
                float* const   t = a.table + 21 * (size_t)(h / 3u) + 3u * (1u + h % 3u);
                t[0] = fx, t[1] = fy, t[2] = fz;
            }
        }
    }
    pn_count(head, &a.stats[1]);
    pn_count(boundary, &a.stats[2]);
    pn_count(nonmanifold, &a.stats[3]);
    pn_count(inconsistent, &a.stats[4]);
}

// one more stable sort of the pairs in (keys[r], vals[r]) by src[value]; returns the new r
int pn_sort_by(hipStream_t stream, const PseudonormalArgs& a, const uint32_t* src, int r, uint32_t n, bool first)
{
    const uint32_t blocks = (n + kBlock - 1) / kBlock;
    uint32_t* const keys[2] = {a.keys[r], a.keys[r ^ 1]};
    uint32_t* const vals[2] = {a.vals[r], a.vals[r ^ 1]};
    if (first)
        hipLaunchKernelGGL(k_pn_pairs, dim3(blocks), dim3(kBlock), 0, stream, src, keys[0], vals[0], n);
    else
        hipLaunchKernelGGL(k_pn_gather, dim3(blocks), dim3(kBlock), 0, stream, src, (const uint32_t*)vals[0], keys[0], n);
    return r ^ launch_radix_sort_pairs(stream, keys, vals, n, a.hist, a.scan);
}
}  // namespace

size_t pseudonormal_scan_words(uint32_t corners)
{
    const size_t radix = bvh_radix_scan_words(corners), flags = bvh_scan_scratch_words(corners);
    return radix > flags ? radix : flags;
}

void launch_pseudonormals_build(hipStream_t stream, const PseudonormalArgs& a)
{
    const uint32_t t = a.tri_count, n = 3u * t;  // (the caller refuses 3 t >= 2^32)
    if (t == 0) return;
    const uint32_t blocks = (n + kBlock - 1) / kBlock;
    (void)hipMemsetAsync(a.stats, 0, 8 * sizeof(uint32_t), stream);
    (void)hipMemsetAsync(a.table, 0, sizeof(float) * 21 * (size_t)t, stream);  // a degenerate triangle's seven entries stay +0
    hipLaunchKernelGGL(k_pn_setup, dim3((t + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
    int r = pn_sort_by(stream, a, a.kz, 0, n, true);
    r     = pn_sort_by(stream, a, a.ky, r, n, false);
    r     = pn_sort_by(stream, a, a.kx, r, n, false);
    hipLaunchKernelGGL(k_pn_heads, dim3(blocks), dim3(kBlock), 0, stream, a, (const uint32_t*)a.vals[r], n);
    launch_exclusive_scan_u32(stream, a.flag, n, a.scan);
    hipLaunchKernelGGL(k_pn_weld, dim3(blocks), dim3(kBlock), 0, stream, a, (const uint32_t*)a.vals[r], n);
    hipLaunchKernelGGL(k_pn_vertex_sums, dim3(blocks), dim3(kBlock), 0, stream, a, (const uint32_t*)a.vals[r], n);
    hipLaunchKernelGGL(k_pn_halfedges, dim3(blocks), dim3(kBlock), 0, stream, a, n);
    r = pn_sort_by(stream, a, a.kz, r, n, true);
    r = pn_sort_by(stream, a, a.ky, r, n, false);
    hipLaunchKernelGGL(k_pn_edge_sums, dim3(blocks), dim3(kBlock), 0, stream, a, (const uint32_t*)a.vals[r], n);
}
}  // namespace cap
