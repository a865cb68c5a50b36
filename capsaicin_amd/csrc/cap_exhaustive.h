// cap_exhaustive.h — exhaustive intersection of small scenes: the triangle and fan-pair record forms and the three intersectors
// (closest hit, its two-phase marked form, any hit), shared by the queue kernels (kernels.hip), the shading bodies (cap_shade.h)
// and the fused kernel (small_scene.hip).  Device code only.
#pragma once

#include "cap_trace.h"

namespace cap
{
// Small scenes (tri_count <= kExhaustiveMax): the hierarchy degenerates to one leaf holding every triangle, tested
// exhaustively.  The loop counter is wave-uniform, so the triangle records are fetched once per wave through the scalar
// data cache (s_load) instead of 64 times through the vector path, and no lane ever waits for another lane's traversal:
// 64-lane SIMD efficiency is 100 % whatever the ray distribution.  Same hit rule, so the same answer as the stack traversal.
// The triangle array is written once by the BVH build and never during a render, so it may be read through the constant
// address space: with a wave-uniform index the compiler then emits s_load (scalar data cache, operands in SGPRs).
struct RawF4
{
    float x, y, z, w;
};
struct alignas(64) RawTri
{
    RawF4 q[4];
};
// One 64-byte triangle record per s_load_dwordx16.
__device__ __forceinline__ void load_const_tri(const float4* base, uint32_t k, float4& t0, float4& t1, float4& t2, float4& t3)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const RawTri ConstTri;
    const RawTri v = ((const ConstTri*)base)[k];
    t0 = make_float4(v.q[0].x, v.q[0].y, v.q[0].z, v.q[0].w);
    t1 = make_float4(v.q[1].x, v.q[1].y, v.q[1].z, v.q[1].w);
    t2 = make_float4(v.q[2].x, v.q[2].y, v.q[2].z, v.q[2].w);
    t3 = make_float4(v.q[3].x, v.q[3].y, v.q[3].z, v.q[3].w);
#else
    t0 = base[4 * k], t1 = base[4 * k + 1], t2 = base[4 * k + 2], t3 = base[4 * k + 3];
#endif
}

// The two sign flips of tri_scaled(), each as one v_bitop3_b32 on the device.  With K = 0x80000000 and s = f2u(ddn) & K:
//   CAP_FLIP_SAME(s, x) = x ^ s        = x ^ (ddn & K)     (V, whose own negation is folded in: see tri_scaled)
//   CAP_FLIP_OPP(s, x)  = x ^ (s ^ K)  = x ^ (~ddn & K)    (U and T)
// Truth table of bitop3(a, b, c, TABLE): bit i of the result is TABLE's bit (a_i << 2 | b_i << 1 | c_i), i.e. TABLE is the expression
// evaluated on a = 0xf0, b = 0xcc, c = 0xaa.  With (a, b, c) = (ddn, x, K): 0xcc ^ (0xf0 & 0xaa) = 0xcc ^ 0xa0 = 0x6c and
// 0xcc ^ (~0xf0 & 0xaa) = 0xcc ^ 0x0a = 0xc6.  The same bit function as the plain expression, which the compiler turns into a v_xor
// with K followed by a 0x6c bitop3 inside the loops (and canonicalises `~f2u(ddn) & K` back to); the builtin is kept as written, and
// ddn goes in unmasked -- as does a sign word that is masked already (PairPre).  -DCAP_MARK_V1 and host code keep the plain expressions.
// Macros, not functions: inside a function of its own the optimiser rewrites the plain x ^ (s ^ K) as a negation of x ^ s before it
// is inlined, and the -DCAP_MARK_V1 build would no longer be the parent's code.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(CAP_MARK_V1)
#define CAP_SIGN_WORD(ddn) f2u(ddn)
#define CAP_FLIP_SAME(s, x) u2f(__builtin_amdgcn_bitop3_b32((s), f2u(x), 0x80000000u, 0x6c))
#define CAP_FLIP_OPP(s, x) u2f(__builtin_amdgcn_bitop3_b32((s), f2u(x), 0x80000000u, 0xc6))
#else
#define CAP_SIGN_WORD(ddn) (f2u(ddn) & 0x80000000u)
#define CAP_FLIP_SAME(s, x) u2f(f2u(x) ^ (s))
#define CAP_FLIP_OPP(s, x) u2f(f2u(x) ^ ((s) ^ 0x80000000u))
#endif

// The determinant-scaled quantities of tri_test() for one triangle record, sign-flipped so that det >= 0.  Same values bit for
// bit: det = -(d.n) and V = -(e1.q) are exact negations, so their sign bits are folded into the flip masks instead of being
// applied first (three bit operations instead of five).
struct TriScaled
{
    float det, U, V, T;  // det = |d.n|
};
__device__ __forceinline__ TriScaled tri_scaled(const Ray& r, const float4 t0, const float4 t1, const float4 t2)
{
    const v3 v0 = mk3(t0.x, t0.y, t0.z), e1 = mk3(t0.w, t1.x, t1.y), e2 = mk3(t1.z, t1.w, t2.x), n = mk3(t2.y, t2.z, t2.w);
    const v3 tvec = r.o - v0;
    const v3 q    = cross3(tvec, r.d);
    const float    ddn = dot3(r.d, n);  // det = -ddn
    const uint32_t s   = CAP_SIGN_WORD(ddn);  // sign of ddn = NOT sign of det
    TriScaled      o;
    o.det = fabsf(ddn);
    o.U   = CAP_FLIP_OPP(s, dot3(e2, q));   // U ^ sign(det)
    o.V   = CAP_FLIP_SAME(s, dot3(e1, q));  // (-e1.q) ^ sign(det)
    o.T   = CAP_FLIP_OPP(s, dot3(tvec, n));
    return o;
}

// Fan pair: triangles id and id + 1 share v0 and the edge e2(id) == e1(id + 1) (every triangulated quad), so tvec, q and that
// edge's dot product with q are computed once.  20 floats: (v0, e1, e2, e3, nA, nB, asfloat(id), 0), read through the scalar
// cache like the single records.  The per-triangle arithmetic is exactly tri_scaled()'s.
struct alignas(16) RawPair
{
    float f[20];
};
struct PairScaled
{
    TriScaled a, b;
    uint32_t  id;
};
// ORG: every ray of the launch has the same origin (camera rays), so tvec = o - v0 and T = tvec.n of both triangles are the same
// for every ray; org_tab holds them per pair -- (tvec, tvec.nA) (tvec.nB, -, -, -), computed once per workgroup with the operations
// below -- and the loop reads them from LDS (one address for the whole wave) instead of spending nine vector instructions.
template <bool ORG = false>
__device__ __forceinline__ PairScaled pair_scaled(const Ray& r, const float4* base, uint32_t k, const float4* org_tab = nullptr)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const RawPair ConstPair;
    const RawPair p = ((const ConstPair*)base)[k];
#else
    RawPair p;
    for (int i = 0; i < 20; ++i) p.f[i] = reinterpret_cast<const float*>(base)[20 * k + i];
#endif
    const v3 v0 = mk3(p.f[0], p.f[1], p.f[2]), e1 = mk3(p.f[3], p.f[4], p.f[5]), e2 = mk3(p.f[6], p.f[7], p.f[8]),
             e3 = mk3(p.f[9], p.f[10], p.f[11]), na = mk3(p.f[12], p.f[13], p.f[14]), nb = mk3(p.f[15], p.f[16], p.f[17]);
    v3    tvec;
    float tna, tnb;
    if (ORG)
    {
        const float4 c0 = org_tab[2 * k], c1 = org_tab[2 * k + 1];
        tvec = mk3(c0.x, c0.y, c0.z), tna = c0.w, tnb = c1.x;
    }
    else
        tvec = r.o - v0, tna = dot3(tvec, na), tnb = dot3(tvec, nb);
    const v3 q    = cross3(tvec, r.d);
    const float e2q = dot3(e2, q);  // U of the first triangle, V (before its negation) of the second
    PairScaled  o;
    {
        const float    ddn = dot3(r.d, na);
        const uint32_t s   = CAP_SIGN_WORD(ddn);
        o.a.det = fabsf(ddn);
        o.a.U   = CAP_FLIP_OPP(s, e2q);
        o.a.V   = CAP_FLIP_SAME(s, dot3(e1, q));
        o.a.T   = CAP_FLIP_OPP(s, tna);
    }
    {
        const float    ddn = dot3(r.d, nb);
        const uint32_t s   = CAP_SIGN_WORD(ddn);
        o.b.det = fabsf(ddn);
        o.b.U   = CAP_FLIP_OPP(s, dot3(e3, q));
        o.b.V   = CAP_FLIP_SAME(s, e2q);
        o.b.T   = CAP_FLIP_OPP(s, tnb);
    }
    o.id = f2u(p.f[18]);
    return o;
}

// Exhaustive closest hit.  Same rule as tri_test() + "minimum t, ties to the lower id": both record lists are in ascending id
// order, so within a list "first strictly smaller t" is that rule (an equal t never replaces an earlier triangle); the two
// lists' winners are merged by the explicit (t, id) order.  With best_t starting at tmax, t < best_t implies t < tmax.  Only t
// and the id are tracked in the loops; the barycentrics of the winner are recomputed once afterwards (identical operations,
// identical bits) instead of being multiplied out and selected for every triangle.
// One candidate per triangle: its t, or +inf when the ray misses it.  Four triangles are tested side by side and reduced by
// a tree instead of a sequential compare chain (measured faster: more independent instructions for the scheduler to
// interleave); "(t, id) lexicographic minimum" is associative, so the tree gives the winner of the sequential rule.
// rec_tab: where the winner's record is re-read from (bvh.tris_by_id, or its LDS copy).
// MANY: the scene may hold more than 32 fan pairs (only in forced exhaustive mode beyond kExhaustiveMax triangles)
template <bool ORG = false, bool MANY = true>
__device__ __forceinline__ void exhaustive_closest(const BvhDev& bvh, const float4* rec_tab, const Ray& r, float& best_t, float& best_u,
                                                   float& best_v, uint32_t& best_gid, const float4* org_tab = nullptr,
                                                   uint32_t pair_mask = ~0u)
{
    best_t = r.tmax, best_u = 0.0f, best_v = 0.0f, best_gid = kInvalidId;
    auto cand = [&](const TriScaled& s) {
        const bool  inside = (s.U >= 0.0f) & (s.V >= 0.0f) & (s.U + s.V <= s.det);
        const float tt     = s.T * rcp_c(s.det);
        return (inside & (tt > r.tmin)) ? tt : __builtin_inff();
    };
    // ---- fan pairs, two at a time ----
    // A ray is inside at most one triangle of a planar quad except on the shared diagonal, so a pair needs one reciprocal: of the
    // triangle the ray is inside of.  Its t is bit for bit the one the per-triangle rule computes; the other triangle's
    // candidate is +inf either way.  Pairs some lane is inside both triangles of (non-planar fans, rays on the diagonal) take
    // the two-reciprocal form for the whole wave (wave-uniform branch, rare).
    auto pair_cand = [&](const PairScaled& p, float& m, uint32_t& im) {
        const bool a0 = p.a.U >= 0.0f, a1 = p.a.V >= 0.0f, a2 = p.a.U + p.a.V <= p.a.det;
        const bool b0 = p.b.U >= 0.0f, b1 = p.b.V >= 0.0f, b2 = p.b.U + p.b.V <= p.b.det;
        const bool ia = a0 & a1 & a2, ib = b0 & b1 & b2;
        // "some lane is inside both": the six compares' own lane masks AND-ed in scalar registers.  The ballot of the computed bool
        // (ia & ib) instead costs four half-rate vector instructions per pair -- two 0 / 1 materialisations, an AND and a compare -- and
        // keeps the 0 / 1 words alive for the compiler to build (ia | ib) and the id from: 20 issue cycles of a pair's ~165 (round 6, (87)).
        const unsigned long long both = __builtin_amdgcn_ballot_w64(a0) & __builtin_amdgcn_ballot_w64(a1) & __builtin_amdgcn_ballot_w64(a2) &
                                        __builtin_amdgcn_ballot_w64(b0) & __builtin_amdgcn_ballot_w64(b1) & __builtin_amdgcn_ballot_w64(b2);
        if (__builtin_expect(both != 0ull, 0))
        {
            const float ta = p.a.T * rcp_c(p.a.det), tb = p.b.T * rcp_c(p.b.det);
            const float ca = (ia & (ta > r.tmin)) ? ta : __builtin_inff(), cb = (ib & (tb > r.tmin)) ? tb : __builtin_inff();
            const bool  pb = cb < ca;  // strict: the earlier triangle keeps an equal t
            m = pb ? cb : ca, im = pb ? p.id + 1u : p.id;
        }
        else
        {
            const float tt = (ib ? p.b.T : p.a.T) * rcp_c(ib ? p.b.det : p.a.det);
            m  = ((ia | ib) & (tt > r.tmin)) ? tt : __builtin_inff();
            im = ib ? p.id + 1u : p.id;
        }
    };
    // pair_mask (wave-uniform): the fan pairs some ray of the wave can reach at all (camera rays: the pairs whose screen bounds
    // overlap the wave's tile, k_trace_shade); visited in ascending order, like the full list
    const uint32_t np = bvh.fan_pair_count;
    uint32_t       pm = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pair_mask & (np >= 32u ? ~0u : ((1u << np) - 1u))));
    if (MANY && np > 32u)
    {
        // more pairs than the mask holds (forced exhaustive mode on a larger scene): every pair, two at a time
        pm         = 0u;
        uint32_t k = 0;
        for (; k + 2 <= np; k += 2)
        {
            const PairScaled p0 = pair_scaled<ORG>(r, bvh.fan_pairs, k, org_tab), p1 = pair_scaled<ORG>(r, bvh.fan_pairs, k + 1, org_tab);
            float            m01, m23;
            uint32_t         i01, i23;
            pair_cand(p0, m01, i01);
            pair_cand(p1, m23, i23);
            const bool     p  = m23 < m01;
            const float    m  = p ? m23 : m01;
            const uint32_t im = p ? i23 : i01;
            const bool     better = m < best_t;
            best_t   = better ? m : best_t;
            best_gid = better ? im : best_gid;
        }
        if (k < np)
        {
            const PairScaled p0 = pair_scaled<ORG>(r, bvh.fan_pairs, k, org_tab);
            float            m;
            uint32_t         im;
            pair_cand(p0, m, im);
            const bool better = m < best_t;
            best_t   = better ? m : best_t;
            best_gid = better ? im : best_gid;
        }
    }
    while (pm != 0u)
    {
        const uint32_t k0 = (uint32_t)__builtin_ctz(pm);
        pm &= pm - 1u;
        if (pm != 0u)
        {
            const uint32_t k1 = (uint32_t)__builtin_ctz(pm);
            pm &= pm - 1u;
            const PairScaled p0 = pair_scaled<ORG>(r, bvh.fan_pairs, k0, org_tab), p1 = pair_scaled<ORG>(r, bvh.fan_pairs, k1, org_tab);
            float            m01, m23;
            uint32_t         i01, i23;
            pair_cand(p0, m01, i01);
            pair_cand(p1, m23, i23);
            const bool     p  = m23 < m01;
            const float    m  = p ? m23 : m01;
            const uint32_t im = p ? i23 : i01;
            const bool     better = m < best_t;
            best_t   = better ? m : best_t;
            best_gid = better ? im : best_gid;
        }
        else
        {
            const PairScaled p0 = pair_scaled<ORG>(r, bvh.fan_pairs, k0, org_tab);
            float            m;
            uint32_t         im;
            pair_cand(p0, m, im);
            const bool better = m < best_t;
            best_t   = better ? m : best_t;
            best_gid = better ? im : best_gid;
        }
    }
    // ---- unpaired triangles ----
    const uint32_t ns = bvh.fan_single_count;
    if (ns)
    {
        float    st = r.tmax;
        uint32_t si = kInvalidId;
#pragma unroll 2
        for (uint32_t j = 0; j < ns; ++j)
        {
            float4 t0, t1, t2, t3;
            load_const_tri(bvh.fan_singles, j, t0, t1, t2, t3);
            const float c      = cand(tri_scaled(r, t0, t1, t2));
            const bool  better = c < st;
            st = better ? c : st;
            si = better ? f2u(t3.x) : si;
        }
        const bool better = (st < best_t) | ((st == best_t) & (si < best_gid));
        best_t   = better ? st : best_t;
        best_gid = better ? si : best_gid;
    }
    if (best_gid != kInvalidId)
    {
        const float4*   rec = rec_tab + 4 * (size_t)best_gid;
        const TriScaled s   = tri_scaled(r, rec[0], rec[1], rec[2]);
        const float     inv = rcp_c(s.det);
        best_u = s.U * inv, best_v = s.V * inv;
    }
}

// Two-phase form of exhaustive_closest() for the LDS-resident small-scene kernels of bounce >= 1 (k_trace_shade, LDS && !ORG;
// -DCAP_CLOSEST_V1 keeps the one-phase form there for A/B runs: tools/build_variant.sh closestv1 -DCAP_CLOSEST_V1).
// About 26 of the pair loop's 58 vector instructions only produce t = T * rcp_c(det) and the running (t, id) minimum, for all 64
// lanes and every triangle, while a lane is inside 2.6-2.8 of the Cornell box's 32 triangles (whole line, either sign of t).
// Phase 1 (wave-uniform, the counted loop over the records through the scalar cache): the inside test alone -- tvec, q, the three
// edge products, the two d.n with their sign words, six compares -- recorded per lane as one bit per GLOBAL triangle id.
// Phase 2 (per lane): for every marked id in ascending order, v0 and n from the LDS copy of tris_by_id, T, det and
// t = T * rcp_c(det) with tri_scaled()'s operations and operand order -- bit for bit the value the one-phase loop computes --
// accepted when t > tmin and t < best_t, strict: ascending ids with a strict compare are "minimum t, ties to the lower id".
// WIDE: more than 32 triangles (up to kExhaustiveMax = 64): two mask words; wave-uniform, chosen once per launch.
// has_ray: false for the lanes past the end of a class's last chunk; they mark nothing.
struct PairInside
{
    bool     a, b;
    uint32_t id;
};
__device__ __forceinline__ bool tri_inside(float ddn, float e2q_u, float e1q_v)
{
    // tri_scaled()'s det, U and V (V = -(e1.q): its negation is folded into the flip mask there and here)
    const uint32_t s   = CAP_SIGN_WORD(ddn);
    const float    det = fabsf(ddn);
    const float    U   = CAP_FLIP_OPP(s, e2q_u);
    const float    V   = CAP_FLIP_SAME(s, e1q_v);
    return (U >= 0.0f) & (V >= 0.0f) & (U + V <= det);
}
__device__ __forceinline__ PairInside pair_inside(const Ray& r, const float4* base, uint32_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const RawPair ConstPair;
    const RawPair p = ((const ConstPair*)base)[k];
#else
    RawPair p;
    for (int i = 0; i < 20; ++i) p.f[i] = reinterpret_cast<const float*>(base)[20 * k + i];
#endif
    const v3 v0 = mk3(p.f[0], p.f[1], p.f[2]), e1 = mk3(p.f[3], p.f[4], p.f[5]), e2 = mk3(p.f[6], p.f[7], p.f[8]),
             e3 = mk3(p.f[9], p.f[10], p.f[11]), na = mk3(p.f[12], p.f[13], p.f[14]), nb = mk3(p.f[15], p.f[16], p.f[17]);
    const v3    tvec = r.o - v0;
    const v3    q    = cross3(tvec, r.d);
    const float e2q  = dot3(e2, q);  // as in pair_scaled(): U of the first triangle, V (before its negation) of the second
    PairInside  o;
    o.a  = tri_inside(dot3(r.d, na), e2q, dot3(e1, q));
    o.b  = tri_inside(dot3(r.d, nb), dot3(e3, q), e2q);
    o.id = f2u(p.f[18]);
    return o;
}
// Phase 1 of a DENSE scene (BvhDev::tri_ids_dense: fan pairs only and pair j holds triangles 2j and 2j + 1, so a triangle's id is its
// position in the list -- every scene made of quads, the Cornell box among them).  No bit word is built from the id: the list is
// walked from its last triangle to its first and every triangle shifts its inside bit in from the right,
//     m = 2 m + inside      one v_addc_co_u32 m, -, m, m, <lane mask>: the carry-in IS the compares' lane mask,
// so after tri_count steps triangle i sits in bit i, the mask the id-indexed form builds (the bits above tri_count are the zeros m started
// with).  The lane mask is the AND of the three compares' own ballots (scalar; a ballot of the computed bool would cost a select and a
// compare per triangle again, experiment (87)) and is the instruction's one scalar operand.  Against the id-indexed form: per pair two
// vector instructions instead of five (2 v_mov of a bit word, 2 v_cndmask, v_or3) and none of the three scalar ones that made the bit words.
// Two words (33-64 triangles): the low word's carry-out is the high word's carry-in.  Both steps of a pair are one asm statement: the
// compiler pads after every statement whose outputs the next instruction reads.  -DCAP_MARK_V1 compiles the id-indexed form alone.
#if defined(CAP_MARK_V1)
constexpr bool kMarkCarry = false;
#else
constexpr bool kMarkCarry = true;
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !defined(CAP_MARK_V1)
__device__ __forceinline__ unsigned long long tri_inside_lanes(float ddn, float e2q_u, float e1q_v)
{
    const uint32_t s   = CAP_SIGN_WORD(ddn);
    const float    det = fabsf(ddn);
    const float    U   = CAP_FLIP_OPP(s, e2q_u);
    const float    V   = CAP_FLIP_SAME(s, e1q_v);
    return __builtin_amdgcn_ballot_w64(U >= 0.0f) & __builtin_amdgcn_ballot_w64(V >= 0.0f) & __builtin_amdgcn_ballot_w64(U + V <= det);
}
// the pair at rec (scalar loads, as pair_inside): its second triangle shifted in, then its first
template <bool WIDE>
__device__ __forceinline__ void pair_shift_in(const Ray& r, const __attribute__((address_space(4))) RawPair* rec, uint32_t& m0, uint32_t& m1)
{
    const RawPair p = *rec;
    const v3 v0 = mk3(p.f[0], p.f[1], p.f[2]), e1 = mk3(p.f[3], p.f[4], p.f[5]), e2 = mk3(p.f[6], p.f[7], p.f[8]),
             e3 = mk3(p.f[9], p.f[10], p.f[11]), na = mk3(p.f[12], p.f[13], p.f[14]), nb = mk3(p.f[15], p.f[16], p.f[17]);
    const v3    tvec = r.o - v0;
    const v3    q    = cross3(tvec, r.d);
    const float e2q  = dot3(e2, q);
    const unsigned long long ia = tri_inside_lanes(dot3(r.d, na), e2q, dot3(e1, q));
    const unsigned long long ib = tri_inside_lanes(dot3(r.d, nb), dot3(e3, q), e2q);
    unsigned long long       c;  // carry out: between the two words, otherwise unused (always 0 in the high word: <= 64 steps)
    if (WIDE)
        asm("v_addc_co_u32_e64 %0, %2, %0, %0, %3\n\tv_addc_co_u32_e64 %1, %2, %1, %1, %2\n\t"
            "v_addc_co_u32_e64 %0, %2, %0, %0, %4\n\tv_addc_co_u32_e64 %1, %2, %1, %1, %2"
            : "+v"(m0), "+v"(m1), "=&s"(c)
            : "s"(ib), "s"(ia));
    else
        asm("v_addc_co_u32_e64 %0, %1, %0, %0, %2\n\tv_addc_co_u32_e64 %0, %1, %0, %0, %3" : "+v"(m0), "=&s"(c) : "s"(ib), "s"(ia));
}
#endif
template <bool WIDE>
__device__ __forceinline__ void exhaustive_closest_marked(const BvhDev& bvh, const float4* rec_tab, const Ray& r, bool has_ray, float& best_t,
                                                          float& best_u, float& best_v, uint32_t& best_gid)
{
    best_t = r.tmax, best_u = 0.0f, best_v = 0.0f, best_gid = kInvalidId;
    // ---- phase 1: candidate mask ----
    uint32_t m0 = 0u, m1 = 0u;
    // bit `id` of (m0, m1); id is wave-uniform, so the bit words are scalar and the branch-free two-word form costs selects only
    auto mark = [&](bool inside, uint32_t id) {
        if (WIDE)
        {
            const uint32_t lo = id < 32u ? 1u << id : 0u, hi = id < 32u ? 0u : 1u << (id - 32u);
            m0 |= inside ? lo : 0u, m1 |= inside ? hi : 0u;
        }
        else
            m0 |= inside ? 1u << id : 0u;
    };
    const uint32_t np = bvh.fan_pair_count;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(CAP_MARK_V1)
    if (bvh.tri_ids_dense)  // wave-uniform, the same for the whole launch
    {
        // last pair first, two per iteration (written out: the asm statement defeats #pragma unroll); an odd count's last pair goes first
        const __attribute__((address_space(4))) RawPair* rec = (const __attribute__((address_space(4))) RawPair*)bvh.fan_pairs + np;
        if (np & 1u) pair_shift_in<WIDE>(r, --rec, m0, m1);
        for (uint32_t k = np >> 1; k != 0u; --k)
        {
            pair_shift_in<WIDE>(r, rec - 1, m0, m1);
            pair_shift_in<WIDE>(r, rec - 2, m0, m1);
            rec -= 2;
        }
    }
    else
#endif
    {
#pragma unroll 2
        for (uint32_t k = 0; k < np; ++k)
        {
            const PairInside p = pair_inside(r, bvh.fan_pairs, k);
            mark(p.a, p.id);
            mark(p.b, p.id + 1u);
        }
        const uint32_t ns = bvh.fan_single_count;
#pragma unroll 2
        for (uint32_t j = 0; j < ns; ++j)
        {
            float4 t0, t1, t2, t3;
            load_const_tri(bvh.fan_singles, j, t0, t1, t2, t3);
            const v3 v0 = mk3(t0.x, t0.y, t0.z), e1 = mk3(t0.w, t1.x, t1.y), e2 = mk3(t1.z, t1.w, t2.x), n = mk3(t2.y, t2.z, t2.w);
            const v3 q  = cross3(r.o - v0, r.d);
            mark(tri_inside(dot3(r.d, n), dot3(e2, q), dot3(e1, q)), f2u(t3.x));
        }
    }
    if (!has_ray) m0 = 0u, m1 = 0u;
    // ---- phase 2: the marked triangles of this lane, ascending id ----
    while ((m0 | (WIDE ? m1 : 0u)) != 0u)
    {
        uint32_t id;
        if (WIDE && m0 == 0u)
            id = 32u + (uint32_t)__builtin_ctz(m1), m1 &= m1 - 1u;
        else
            id = (uint32_t)__builtin_ctz(m0), m0 &= m0 - 1u;
        const float4*  rec = rec_tab + 4 * (size_t)id;
        const float4   t0 = rec[0], t2 = rec[2];
        const v3       v0 = mk3(t0.x, t0.y, t0.z), n = mk3(t2.y, t2.z, t2.w);
        const v3       tvec = r.o - v0;
        const float    ddn  = dot3(r.d, n);
        const uint32_t s    = CAP_SIGN_WORD(ddn);
        const float    T    = CAP_FLIP_OPP(s, dot3(tvec, n));
        const float    tt   = T * rcp_c(fabsf(ddn));
        const bool     better = (tt > r.tmin) & (tt < best_t);
        best_t   = better ? tt : best_t;
        best_gid = better ? id : best_gid;
    }
    if (best_gid != kInvalidId)
    {
        const float4*   rec = rec_tab + 4 * (size_t)best_gid;
        const TriScaled s   = tri_scaled(r, rec[0], rec[1], rec[2]);
        const float     inv = rcp_c(s.det);
        best_u = s.U * inv, best_v = s.V * inv;
    }
}

// Everything of the occlusion test that depends on the ray's DIRECTION and the triangle only: sign mask of d.n, |d.n| and the two
// interval bounds tmin * |d.n|, tmax * |d.n|.  The reference model's shadow rays of one frame share the direction (the frame's
// light) and tmin / tmax are constants, so k_trace_any computes these once per (frame slot, fan pair) and workgroup -- the same
// operations on the same operands as pair_scaled() + the occlusion test, hence the same bits -- and the pair loop reads them from
// LDS: ten vector instructions fewer per pair.
struct PairPre
{
    float4 a, b;  // per triangle: (asfloat(sign mask), det, tmin * det, tmax * det)
};
__device__ __forceinline__ float4 tri_pre(const v3 d, const v3 n, float tmin, float tmax)
{
    const float    ddn = dot3(d, n);
    const uint32_t s   = f2u(ddn) & 0x80000000u;
    const float    det = fabsf(ddn);
    return make_float4(u2f(s), det, tmin * det, tmax * det);
}
// pair k of the record list against a ray whose direction-dependent part comes from the table
__device__ __forceinline__ bool pair_occludes_pre(const Ray& r, const float4* base, uint32_t k, const float4 pa, const float4 pb)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const RawPair ConstPair;
    const RawPair p = ((const ConstPair*)base)[k];
#else
    RawPair p;
    for (int i = 0; i < 20; ++i) p.f[i] = reinterpret_cast<const float*>(base)[20 * k + i];
#endif
    const v3 v0 = mk3(p.f[0], p.f[1], p.f[2]), e1 = mk3(p.f[3], p.f[4], p.f[5]), e2 = mk3(p.f[6], p.f[7], p.f[8]),
             e3 = mk3(p.f[9], p.f[10], p.f[11]), na = mk3(p.f[12], p.f[13], p.f[14]), nb = mk3(p.f[15], p.f[16], p.f[17]);
    const v3    tvec = r.o - v0;
    const v3    q    = cross3(tvec, r.d);
    const float e2q  = dot3(e2, q);
    bool        hit;
    {
        const uint32_t s = f2u(pa.x);
        const float    U = CAP_FLIP_OPP(s, e2q), V = CAP_FLIP_SAME(s, dot3(e1, q)), T = CAP_FLIP_OPP(s, dot3(tvec, na));
        hit = (U >= 0.0f) & (V >= 0.0f) & (U + V <= pa.y) & (T > pa.z) & (T < pa.w);
    }
    {
        const uint32_t s = f2u(pb.x);
        const float    U = CAP_FLIP_OPP(s, dot3(e3, q)), V = CAP_FLIP_SAME(s, e2q), T = CAP_FLIP_OPP(s, dot3(tvec, nb));
        hit |= (U >= 0.0f) & (V >= 0.0f) & (U + V <= pb.y) & (T > pb.z) & (T < pb.w);
    }
    return hit;
}

// det == 0 needs no test: then U = V = 0 is the only way past the first three conditions and 0 < T < 0 rejects.
// PRE: pre_row is this lane's row of the (frame slot, pair) table (see PairPre)
// NEE: the EXT model's next-event rays walk the list whose tail holds the pairs that cannot occlude them (BvhDev::fan_pairs_nee)
template <bool PRE = false, bool NEE = false>
__device__ __forceinline__ bool exhaustive_any(const BvhDev& bvh, const Ray& r, const float4* pre_row = nullptr)
{
    auto occl = [&](const TriScaled& s) {
        return (s.U >= 0.0f) & (s.V >= 0.0f) & (s.U + s.V <= s.det) & (s.T > r.tmin * s.det) & (s.T < r.tmax * s.det);
    };
    bool                hit  = false;
    const uint32_t      np   = NEE ? bvh.fan_pair_nee_count : bvh.fan_pair_count;
    const float4* const list = NEE ? bvh.fan_pairs_nee : bvh.fan_pairs;
#pragma unroll 2
    for (uint32_t k = 0; k < np; ++k)
    {
        if (PRE)
            hit |= pair_occludes_pre(r, list, k, pre_row[2 * k], pre_row[2 * k + 1]);
        else
        {
            const PairScaled p = pair_scaled(r, list, k);
            hit |= occl(p.a) | occl(p.b);
        }
    }
    const uint32_t ns = bvh.fan_single_count;
#pragma unroll 2
    for (uint32_t j = 0; j < ns; ++j)
    {
        float4 t0, t1, t2, t3;
        load_const_tri(bvh.fan_singles, j, t0, t1, t2, t3);
        hit |= occl(tri_scaled(r, t0, t1, t2));
    }
    return hit;
}
}  // namespace cap
