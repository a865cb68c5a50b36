// cap_near.h — the arithmetic closest-point queries over instances (cap_closest_instances) prune with, host and device: the
// per-instance world-to-object data of k_instance_setup (instance.hip), the two values the distance prune adds to it (g, Xw), the
// per-point slack and the skip predicate of k_closest_inst (point_query.hip).  cap_debug_closest_instance_bound (context.hip) runs the
// same functions on the host, so that the CPU tests exercise what ships.  DESIGN.md "Closest-point queries over instances" has the
// argument for the constants.  At the end: the same for box overlap queries over instances (cap_overlap_instances) -- the slack, the
// object-space image of a world box and the skip test of k_overlap_inst (overlap.hip), which cap_debug_overlap_instance_prune runs.
#pragma once

#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace cap
{
constexpr float kNearEps = 5.9604644775390625e-8f;  // 2^-24
constexpr float kNearC1  = 16.0f;                   // relative part of the bound: the proof needs 10.1, the bound's own roundings 4
constexpr float kNearC2  = 96.0f;                   // slack = kNearC2 eps (|p|_inf + Xw): the proof needs 85

__host__ __device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }
__host__ __device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.40282347e38f; }

// inverse of the affine map m (row-major 3x4) in double; false when it is singular or the result is not finite
__host__ __device__ __forceinline__ bool invert_affine(const double m[12], double w[12])
{
    const double c00 = m[5] * m[10] - m[6] * m[9], c01 = m[6] * m[8] - m[4] * m[10], c02 = m[4] * m[9] - m[5] * m[8];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    if (!(fabs(det) > 0.0) || !finite_d(det)) return false;
    const double id = 1.0 / det;
    w[0] = c00 * id, w[1] = (m[2] * m[9] - m[1] * m[10]) * id, w[2] = (m[1] * m[6] - m[2] * m[5]) * id;
    w[4] = c01 * id, w[5] = (m[0] * m[10] - m[2] * m[8]) * id, w[6] = (m[2] * m[4] - m[0] * m[6]) * id;
    w[8] = c02 * id, w[9] = (m[1] * m[8] - m[0] * m[9]) * id, w[10] = (m[0] * m[5] - m[1] * m[4]) * id;
    bool ok = true;
    for (int r = 0; r < 3; ++r)
    {
        w[4 * r + 3] = -(w[4 * r] * m[3] + w[4 * r + 1] * m[7] + w[4 * r + 2] * m[11]);
        for (int k = 0; k < 4; ++k) ok = ok && finite_d(w[4 * r + k]);
    }
    return ok;
}
__host__ __device__ __forceinline__ double norm_inf3(const double m[12])
{
    double n = 0.0;
    for (int r = 0; r < 3; ++r) n = fmax(n, fabs(m[4 * r]) + fabs(m[4 * r + 1]) + fabs(m[4 * r + 2]));
    return n;
}

// What an instance's transform m (binary32 entries held in double; live = they are finite and the object exists) gives every instanced
// query: w = inverse(m) in double, wf = fl32(w) -- the stored W --, wd = wf in double, A = inverse(wd), kappa = |A| |wd| (row-sum norms).
// Returns whether the instance is live (include/capsaicin_hip.h "Inert instances"); wf is all zero otherwise.
__host__ __device__ __forceinline__ bool instance_inverse(const double m[12], bool live, double w[12], float wf[12], double wd[12], double A[12],
                                                          double& nA, double& kappa, float max_condition)
{
    live = live && invert_affine(m, w);
    for (int k = 0; k < 12; ++k) wf[k] = live ? (float)w[k] : 0.0f, wd[k] = (double)wf[k], live = live && finite_f(wf[k]);
    live  = live && invert_affine(wd, A);
    nA    = live ? norm_inf3(A) : 0.0;
    kappa = nA * norm_inf3(wd);
    return live && kappa <= (double)max_condition;
}

// g: a lower bound on the smallest singular value of m's 3x3 part, from w = inverse(m) in double.  S = w w^T is rotated towards its
// diagonal by cyclic Jacobi sweeps (orthogonal similarities: the eigenvalues stay), then Gershgorin's discs bound its largest eigenvalue
// from above WHATEVER the sweeps left off the diagonal: sigma_max(w)^2 <= max_i (S_ii + sum_j |S_ij|), and sigma_min(m) = 1 / sigma_max(w).
// The sweeps only make the bound tight (five leave off-diagonal terms far below 1e-6 of the trace).  1e-6 relative is taken off for
// everything done in double here and before (the inverse's own error is kappa x 2^-53, the rotations' a few 2^-53 each) and for the
// rounding to binary32.
__host__ __device__ __forceinline__ float near_sigma_min_bound(const double w[12])
{
    double s[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) s[i][j] = w[4 * i] * w[4 * j] + w[4 * i + 1] * w[4 * j + 1] + w[4 * i + 2] * w[4 * j + 2];
    for (int sweep = 0; sweep < 5; ++sweep)
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q)
            {
                const double apq = s[p][q];
                if (!(fabs(apq) > 0.0)) continue;
                const double theta = (s[q][q] - s[p][p]) / (2.0 * apq);
                const double t     = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                const int    r = 3 - p - q;
                const double app = s[p][p], aqq = s[q][q], arp = s[r][p], arq = s[r][q];
                s[p][p] = app - t * apq, s[q][q] = aqq + t * apq;
                s[p][q] = s[q][p] = 0.0;
                s[r][p] = s[p][r] = c * arp - sn * arq;
                s[r][q] = s[q][r] = sn * arp + c * arq;
            }
    double top = 0.0;
    for (int i = 0; i < 3; ++i) top = fmax(top, fabs(s[i][0]) + fabs(s[i][1]) + fabs(s[i][2]));
    if (!(top > 0.0) || !finite_d(top)) return 0.0f;
    const float g = (float)((1.0 - 1e-6) / sqrt(top));
    return finite_f(g) ? g : 0.0f;
}

// Xw: no world coordinate the contract's record arithmetic meets for a point of the object box [blo, bhi] exceeds it -- per row of m the
// sum of the MAGNITUDES of the terms, so that it also bounds what cancels (an object far from its origin moved back to the world's).
// Rounded upwards.
__host__ __device__ __forceinline__ float near_world_extent(const double m[12], const double blo[3], const double bhi[3])
{
    double x = 0.0;
    for (int r = 0; r < 3; ++r)
    {
        double row = fabs(m[4 * r + 3]);
        for (int k = 0; k < 3; ++k) row += fabs(m[4 * r + k]) * fmax(fabs(blo[k]), fabs(bhi[k]));
        x = fmax(x, row);
    }
    return nextafterf((float)x, INFINITY);
}

// the absolute part of the bound for point p (pmax = |p|_inf) against an instance of world extent xw
__host__ __device__ __forceinline__ float near_slack(float pmax, float xw) { return (kNearC2 * kNearEps) * (pmax + xw); }

// The squared distance beyond which a box is skipped while the best world distance is sqrt_best = sqrtf(best dist2): in world space (the
// top level's boxes), and in the object space of an instance with g <= sigma_min.  Never below best itself; +inf while best is.
__host__ __device__ __forceinline__ float near_bound2_world(float sqrt_best, float slack)
{
    const float b = (sqrt_best + slack) * (1.0f + kNearC1 * kNearEps);
    return (b * b) * (1.0f + 4.0f * kNearEps);
}
__host__ __device__ __forceinline__ float near_bound2_object(float sqrt_best, float slack, float g)
{
    const float b = ((sqrt_best + slack) * (1.0f + kNearC1 * kNearEps)) / g;
    return (b * b) * (1.0f + 4.0f * kNearEps);
}

// p' = W p + W_t, rows w0 .. w2 of the stored W: where the bottom-level boxes are measured from.  Part of the contract of
// cap_signed_distance_instances (include/capsaicin_hip.h), which reads its sign at p': per row
//   p'_r = fl(fl(fl(fl(W_r0 p.x) + fl(W_r1 p.y)) + fl(W_r2 p.z)) + W_r3),
// single rounded binary32 operations in this order, no fused multiply-add.  Do not reorder.
__host__ __device__ __forceinline__ void near_to_object(const float w[12], float px, float py, float pz, float& ox, float& oy, float& oz)
{
    ox = ((w[0] * px + w[1] * py) + w[2] * pz) + w[3];
    oy = ((w[4] * px + w[5] * py) + w[6] * pz) + w[7];
    oz = ((w[8] * px + w[9] * py) + w[10] * pz) + w[11];
}

// squared distance from p to the box [lo, hi], 0 inside
__host__ __device__ __forceinline__ float box_dist2(float px, float py, float pz, float lox, float loy, float loz, float hix, float hiy, float hiz)
{
    const float dx = fmaxf(fmaxf(lox - px, px - hix), 0.f), dy = fmaxf(fmaxf(loy - py, py - hiy), 0.f), dz = fmaxf(fmaxf(loz - pz, pz - hiz), 0.f);
    return (dx * dx + dy * dy) + dz * dz;
}

// the walk's test: a strict >, so that a box at exactly the bound is opened (a NaN distance is opened too)
__host__ __device__ __forceinline__ bool near_skip(float box_d2, float bound2) { return box_d2 > bound2; }

// ---- box overlap queries over instances (cap_overlap_instances, overlap.hip k_overlap_inst) ----
// What the walk prunes with, host and device; cap_debug_overlap_instance_prune (context.hip) runs the same functions.  DESIGN.md "Box
// overlap queries over instances" derives the constant: the argument needs 64, the two roundings of the slack and its division take
// three eps more.
constexpr float kOverlapC2 = 96.0f;

// the largest coordinate magnitude of the query box
__host__ __device__ __forceinline__ float overlap_box_max(float lox, float loy, float loz, float hix, float hiy, float hiz)
{
    return fmaxf(fmaxf(fmaxf(fabsf(lox), fabsf(loy)), fmaxf(fabsf(loz), fabsf(hix))), fmaxf(fabsf(hiy), fabsf(hiz)));
}
// slack_i = c2 eps (|box|_inf + Xw_i): what the world query box is grown by at the top level (xw = the table's largest Xw), and,
// divided by g <= sigma_min, its object-space image inside instance i
__host__ __device__ __forceinline__ float overlap_slack(float bmax, float xw) { return (kOverlapC2 * kNearEps) * (bmax + xw); }

// The object-space image of the world box of centre c and half-extent h (BoxFrame's) under the stored W, grown by s:
//   c'_r = fl(fl(fl(fl(W_r0 c.x) + fl(W_r1 c.y)) + fl(W_r2 c.z)) + W_r3)   (near_to_object),
//   h'_r = fl(fl(fl(|W_r0| h.x) + fl(|W_r1| h.y)) + fl(|W_r2| h.z)),
//   olo_r = fl(fl(c'_r - h'_r) - s),  ohi_r = fl(fl(c'_r + h'_r) + s).
// Plain products and sums; an image that is not finite compares false with everything and so opens every node.
__host__ __device__ __forceinline__ void overlap_image(const float w[12], float cx, float cy, float cz, float hx, float hy, float hz, float s, float olo[3],
                                                       float ohi[3])
{
    float c[3];
    near_to_object(w, cx, cy, cz, c[0], c[1], c[2]);
    for (int r = 0; r < 3; ++r)
    {
        const float h = (fabsf(w[4 * r]) * hx + fabsf(w[4 * r + 1]) * hy) + fabsf(w[4 * r + 2]) * hz;
        olo[r] = (c[r] - h) - s, ohi[r] = (c[r] + h) + s;
    }
}

// The walk's test, at the top level (a stored world box against the world query box grown by the top-level slack) and below an instance
// (a node box of the object's tree against the image): true = the box [blo, bhi] lies beyond [qlo, qhi] on some axis.  Every comparison
// is strict and written "x < y": touching opens, and so does a NaN on either side.
__host__ __device__ __forceinline__ bool overlap_miss(float blox, float bloy, float bloz, float bhix, float bhiy, float bhiz, float qlox, float qloy,
                                                      float qloz, float qhix, float qhiy, float qhiz)
{
    return bhix < qlox || qhix < blox || bhiy < qloy || qhiy < bloy || bhiz < qloz || qhiz < bloz;
}

// ---- triangle overlap queries over instances (cap_overlap_triangles_instances, overlap.hip k_overlap_tri_inst) ----
// The object-space image of the query box is no conservative prune for the triangle predicate (DESIGN.md "Triangle overlap queries over
// instances" has the counterexample), so below an instance the walk maps every node box to WORLD space instead and tests it there.
// The world box of the object-space box [lo, hi] under the transform m (row-major 3x4, M as the caller gave it):
//   c_k = fl(fl(0.5 lo_k) + fl(0.5 hi_k)),  h_k = fl(fl(0.5 hi_k) - fl(0.5 lo_k)),
//   cw_r = fl(fl(fl(fl(M_r0 c_0) + fl(M_r1 c_1)) + fl(M_r2 c_2)) + M_r3),
//   hw_r = fl(fl(fl(|M_r0| h_0) + fl(|M_r1| h_1)) + fl(|M_r2| h_2)),
//   wlo_r = fl(cw_r - hw_r),  whi_r = fl(cw_r + hw_r).
// Plain products and sums in this order, no fused multiply-add; |M| is a source modifier on the device.  The result errs by at most
// 11 eps Xw per component against the exact box of M([lo, hi]); a result that is not finite compares false and opens the node.
// cap_debug_overlap_world_node (context.hip) runs the same function.
__host__ __device__ __forceinline__ void overlap_world_box(const float m[12], float lox, float loy, float loz, float hix, float hiy, float hiz, float wlo[3],
                                                           float whi[3])
{
    const float hlx = lox * 0.5f, hly = loy * 0.5f, hlz = loz * 0.5f, hhx = hix * 0.5f, hhy = hiy * 0.5f, hhz = hiz * 0.5f;
    const float cx = hlx + hhx, cy = hly + hhy, cz = hlz + hhz;
    const float hx = hhx - hlx, hy = hhy - hly, hz = hhz - hlz;
    for (int r = 0; r < 3; ++r)
    {
        const float cw = ((m[4 * r] * cx + m[4 * r + 1] * cy) + m[4 * r + 2] * cz) + m[4 * r + 3];
        const float hw = (fabsf(m[4 * r]) * hx + fabsf(m[4 * r + 1]) * hy) + fabsf(m[4 * r + 2]) * hz;
        wlo[r] = cw - hw, whi[r] = cw + hw;
    }
}

// ---- sphere sweep queries (cap_sweep_spheres, cap_sweep_instances; sweep.hip) ----
// The walk's time comparisons and its box test, host and device: both kernels and cap_debug_sweep_instance_prune (context.hip) run them.
constexpr float kSweepPad  = 1.0f + 8.0f * 5.9604645e-8f;  // the slab test's relative padding
constexpr float kSweepTiny = 1.17549435e-38f;              // ... and its absolute one: the smallest normal number
constexpr float kSweepHuge = 3.40282347e38f;


// the far side of every time comparison of the walk
__host__ __device__ __forceinline__ float sweep_padded(float t) { return t * kSweepPad + kSweepTiny; }

// What a lane keeps of its sweep for the walk: the origin, 1 / d per component and the prune radius
struct SweepRay
{
    float ox, oy, oz, ix, iy, iz, grow;
};

// The ray against the box [lo, hi] grown by grow, over [0, far]: true = not rejected, tn = the entry time (0 inside), xp = the padded
// exit it is compared with.  A component of d that is 0 gives +-inf or, on a plane through o, a NaN, which v_min / v_max drop: that
// slab then constrains nothing it should not.
__host__ __device__ __forceinline__ bool sweep_slab_times(const SweepRay& s, float lox, float loy, float loz, float hix, float hiy, float hiz, float far,
                                                          float& tn, float& xp)
{
    const float ax = ((lox - s.grow) - s.ox) * s.ix, bx = ((hix + s.grow) - s.ox) * s.ix;
    const float ay = ((loy - s.grow) - s.oy) * s.iy, by = ((hiy + s.grow) - s.oy) * s.iy;
    const float az = ((loz - s.grow) - s.oz) * s.iz, bz = ((hiz + s.grow) - s.oz) * s.iz;
    const float en = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.f));
    const float ex = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), far));
    tn             = fminf(en, kSweepHuge);
    xp             = sweep_padded(ex);
    return tn <= xp;
}
__host__ __device__ __forceinline__ bool sweep_slab(const SweepRay& s, float lox, float loy, float loz, float hix, float hiy, float hiz, float far, float& tn)
{
    float xp;
    return sweep_slab_times(s, lox, loy, loz, hix, hiy, hiz, far, tn, xp);
}

// ---- sphere sweep queries over instances (cap_sweep_instances, sweep.hip k_sweep_inst) ----
// The prune radius of a sweep of radius r from an origin with |o|_inf = omax against an instance of world extent xw (the table's largest
// at the top level): R = fl(r + fl(C eps . fl(fl(omax + xw) + r))), what every world box -- the stored ones of the top level, the images
// of the object's node boxes under overlap_world_box below -- is grown by before the slab test of the world ray.  DESIGN.md "Sphere
// sweep queries over instances" counts what it holds: the argument needs 87 of the 128.  cap_debug_sweep_instance_prune runs the same
// function.
constexpr float kSweepInstC = 128.0f;
__host__ __device__ __forceinline__ float sweep_prune_radius(float r, float omax, float xw) { return r + (kSweepInstC * kNearEps) * ((omax + xw) + r); }
}  // namespace cap
