// small_scene.hip — the fused stage of the small-scene path (scenes traced exhaustively, cap_exhaustive.h): k_trace_shade, its
// launcher, the per-phase clocks of the diagnostic build and the device self-test of the unscaled shading forms.
#include "cap_shade.h"

#include <cassert>

namespace cap
{
// Fused stage of the small-scene path: closest-hit (exhaustive, wave-uniform) + shading of the vertex it finds, in one pass over
// the ray queue.  The hit record never travels through HBM and the shading stage's memory latency hides under the ALU-bound
// triangle loop of the other waves.  FIRST generates the camera ray instead of reading a queue entry (rt_primary_visibility).
#ifndef CAP_TS_FIRST
#define CAP_TS_FIRST 5  // workgroups per CU the bounce-0 kernel is register-allocated for
#endif
#ifndef CAP_TS_EXT
#define CAP_TS_EXT 6  // ... and the EXT model's bounce >= 1 kernel
#endif
#ifndef CAP_TS_NEXT
#define CAP_TS_NEXT 6  // ... and the bounce >= 1 kernel (8 fits in 64 VGPRs without spills but measured 8 % slower)
#endif
#ifdef CAP_STAMPS
__device__ unsigned long long g_wave_times[2 * 16384];  // (start, end) s_memrealtime of every wave of the LAST fused launch
#endif
// What one instantiation of k_trace_shade is: everything the kernel derives from its five template arguments, derived once.
// shade_prefetch() and shade_vertex() read the same type (cap_shade.h, C).
// LDS: scenes of at most kExhaustiveMax triangles keep their shading records (96 B each) and intersection records in LDS
// (<= 10 KB per workgroup), so the gathers by hit triangle after the loop are ds_reads instead of a global round trip.
// TAME: the scene's shading records are tame (SceneDev::shade_tame, established where they are written), which is what lets the
// vertex's normalize3 -- and with it everything downstream of a unit normal -- take the unscaled forms.  Chosen at launch like LDS;
// only the reference model's kernels with the scene in LDS have the instantiation.
// CODE: ShadeArgs::code_in_color, bounce 0's form without the direct plane.  Only the TAME kernel has it (trace_shade_has_code_form).
template <bool FIRST_, bool EXT_, bool FB_, bool LDS_, bool TAME_, bool CODE_ = false>
struct TraceShadeCfg
{
    static_assert(!TAME_ || (!EXT_ && !FB_ && LDS_), "TAME: reference model, scene in LDS");
    static_assert(!CODE_ || (FIRST_ && TAME_), "CODE: bounce 0 of the reference model, scene in LDS, tame records");
    static constexpr bool FIRST = FIRST_, EXT = EXT_, FB = FB_, LDS = LDS_, TAME = TAME_, CODE = CODE_;
    static constexpr bool CARRY = !EXT, SKY_RMW = false;
    static constexpr bool PROBE = !EXT && !FB && LDS;  // the producer-side shadow probe (ShadeArgs::inline_probe) and the per-wave ring
    // the lean per-chunk plumbing (see kChunkLean): the reference model's kernels with the scene in LDS and tame records.  (The
    // instantiations without TAME pay for it with 8 and 4 B of scratch, the EXT and feedback kernels were not tried: they keep round 8's.)
    static constexpr bool LEAN = PROBE && TAME && kChunkLean;
    static constexpr bool ORG  = FIRST && LDS;  // camera rays of a small scene: per-pair origin terms and screen bounds (stage_camera_pairs)
    static constexpr bool XT   = EXT && LDS;    // EXT model: materials, light table and per-light records (stage_ext_tables)
    static constexpr int  kBlocksPerCu = FB ? 4 : (EXT ? (FIRST ? 5 : CAP_TS_EXT) : (FIRST ? CAP_TS_FIRST : CAP_TS_NEXT));  // launch bounds
};

// ---- the kernel's prologue: what a workgroup stages in LDS once, block by block.  Each function fills the arrays it is given; the
// barrier between them and the chunk loop is stage_frames' (stage_probe_rows has two of its own).
// LDS: the scene's shading and intersection records
__device__ __forceinline__ void stage_scene_records(const BvhDev& bvh, const ShadeArgs& a, float4* lds_shade, float4* lds_rec)
{
    const uint32_t n = bvh.tri_count <= kExhaustiveMax ? bvh.tri_count : kExhaustiveMax;
    for (uint32_t k = threadIdx.x; k < kShadeRec * n; k += kBlock) lds_shade[k] = a.scene.shade_tris[k];
    for (uint32_t k = threadIdx.x; k < 4 * n; k += kBlock) lds_rec[k] = bvh.tris_by_id[k];
}
// XT: the tables of ExtTables, when they fit
__device__ __forceinline__ void stage_ext_tables(const ShadeArgs& a, float* lds_mat, float* lds_lcdf, float4* lds_lrec)
{
    const float* ms = reinterpret_cast<const float*>(a.scene.materials);
    for (uint32_t k = threadIdx.x; k < 12u * a.scene.material_count; k += kBlock) lds_mat[k] = ms[k];
    for (uint32_t k = threadIdx.x; k < a.scene.light_count; k += kBlock)
    {
        lds_lcdf[k] = a.scene.light_cdf[k];
        const float4* lt = a.scene.shade_tris + kShadeRec * (size_t)a.scene.light_tris[k];
        const float4  l0 = lt[0], l1 = lt[1], l2 = lt[2];
        const v3      q0 = mk3(l0.x, l0.y, l0.z), q1 = mk3(l1.x, l1.y, l1.z), q2 = mk3(l2.x, l2.y, l2.z);
        const v3      nl = normalize3(cross3(q1 - q0, q2 - q0));  // as shade_vertex_ext computes it per vertex without the table
        const MaterialDev lm = a.scene.materials[f2u(lt[6].x)];
        lds_lrec[4 * k]     = make_float4(q0.x, q0.y, q0.z, lm.ke[0]);
        lds_lrec[4 * k + 1] = make_float4(q1.x, q1.y, q1.z, lm.ke[1]);
        lds_lrec[4 * k + 2] = make_float4(q2.x, q2.y, q2.z, lm.ke[2]);
        lds_lrec[4 * k + 3] = make_float4(nl.x, nl.y, nl.z, 0.f);
    }
}
// ORG: per fan pair, the origin terms of pair_scaled<ORG> (lds_org) and its pixel bounds (x0, y0, x1, y1) as the launch's camera
// sees it, grown by two pixels (the sub-pixel jitter of the frames and the rounding of the projection); a pair with a vertex at or
// behind the camera plane covers the screen.  A tile of camera rays only tests the pairs whose bounds overlap it: a ray can only hit
// a quad through a sample point inside the quad's projection, so the pairs left out are missed by all 64 rays -- same hits, same bits.
__device__ __forceinline__ void stage_camera_pairs(const BvhDev& bvh, const ShadeArgs& a, float4* lds_org, float4* lds_bounds)
{
    const v3     o  = mk3(a.cam.position[0], a.cam.position[1], a.cam.position[2]);
    const float* fp = reinterpret_cast<const float*>(bvh.fan_pairs);
    for (uint32_t k = threadIdx.x; k < bvh.fan_pair_count && 2 * k + 1 < kExhaustiveMax; k += kBlock)
    {
        const float* rec  = fp + 20 * (size_t)k;  // (v0, e1, e2, e3, nA, nB, id, 0)
        const v3     tvec = o - mk3(rec[0], rec[1], rec[2]);
        lds_org[2 * k]     = make_float4(tvec.x, tvec.y, tvec.z, dot3(tvec, mk3(rec[12], rec[13], rec[14])));
        lds_org[2 * k + 1] = make_float4(dot3(tvec, mk3(rec[15], rec[16], rec[17])), 0.f, 0.f, 0.f);
        // screen bounds: pixel = ((f * (d.right) / (d.forward)) / sensor + 0.5) * extent  (inverse of primary_dir, camera.h:39-63)
        const v3 R = mk3(a.cam.right[0], a.cam.right[1], a.cam.right[2]), U = mk3(a.cam.up[0], a.cam.up[1], a.cam.up[2]),
                 F = mk3(a.cam.forward[0], a.cam.forward[1], a.cam.forward[2]);
        float x0 = 3.0e38f, y0 = 3.0e38f, x1 = -3.0e38f, y1 = -3.0e38f;
        bool  behind = false;
        for (int e = 0; e < 4; ++e)
        {
            const v3    d = e == 0 ? tvec * -1.0f : (mk3(rec[3 * e], rec[3 * e + 1], rec[3 * e + 2]) - tvec);  // vertex - camera
            const float z = dot3(d, F);
            behind |= !(z > 1e-4f);
            const float px = ((a.cam.focal_length * dot3(d, R) / z) / a.cam.sensor_x + 0.5f) * (float)a.screen.width;
            const float py = ((a.cam.focal_length * dot3(d, U) / z) / a.cam.sensor_y + 0.5f) * (float)a.screen.height;
            x0 = fminf(x0, px), x1 = fmaxf(x1, px), y0 = fminf(y0, py), y1 = fmaxf(y1, py);
        }
        const bool usable = a.cull_camera_pairs != 0u && !behind && x0 == x0 && y0 == y0 && x1 == x1 && y1 == y1;
        lds_bounds[k] = usable ? make_float4(x0 - kCameraCullPad, y0 - kCameraCullPad, x1 + kCameraCullPad, y1 + kCameraCullPad) : make_float4(-3.0e38f, -3.0e38f, 3.0e38f, 3.0e38f);
    }
}
// PROBE: the pair whose four vertices reach farthest along the batch's first light direction (k_trace_any_small's first probe) into
// probe_k, and its PairPre rows per frame slot into lds_probe
__device__ __forceinline__ void stage_probe_rows(const BvhDev& bvh, const ShadeArgs& a, float* lds_pscore, uint32_t& probe_k, float4* lds_probe)
{
    const uint32_t np = bvh.fan_pair_count;  // 1 .. kExhaustiveMax / 2, checked by the host
    const float*   fp = reinterpret_cast<const float*>(bvh.fan_pairs);
    if (threadIdx.x < np)
    {
        const float* rec = fp + 20 * (size_t)threadIdx.x;
        const v3     L   = mk3(a.frames[0].light_dir[0], a.frames[0].light_dir[1], a.frames[0].light_dir[2]);
        const v3     v0  = mk3(rec[0], rec[1], rec[2]);
        float        sc  = dot3(v0, L);
        for (int e = 0; e < 3; ++e) sc += dot3(v0 + mk3(rec[3 + 3 * e], rec[4 + 3 * e], rec[5 + 3 * e]), L);
        lds_pscore[threadIdx.x] = sc;
    }
    __syncthreads();
    if (threadIdx.x < np)
    {
        const float sc   = lds_pscore[threadIdx.x];
        uint32_t    rank = 0;
        for (uint32_t j = 0; j < np; ++j)
        {
            const float o = lds_pscore[j];
            rank += (o > sc || (o == sc && j < threadIdx.x)) ? 1u : 0u;
        }
        if (rank == 0) probe_k = threadIdx.x;
    }
    __syncthreads();
    const float* rec = fp + 20 * (size_t)probe_k;
    for (uint32_t sl = threadIdx.x; sl < a.n_slots && sl < kMaxFrameSlots; sl += kBlock)
    {
        const v3 d = mk3(a.frames[sl].light_dir[0], a.frames[sl].light_dir[1], a.frames[sl].light_dir[2]);
        lds_probe[2 * sl]     = tri_pre(d, mk3(rec[12], rec[13], rec[14]), kRayEps, kRayFar);
        lds_probe[2 * sl + 1] = tri_pre(d, mk3(rec[15], rec[16], rec[17]), kRayEps, kRayFar);
    }
}

template <bool FIRST, bool EXT, bool FB = false, bool LDS = false, bool TAME = false, bool CODE = false>
__global__ __launch_bounds__(kBlock, (TraceShadeCfg<FIRST, EXT, FB, LDS, TAME, CODE>::kBlocksPerCu)) void k_trace_shade(BvhDev bvh, ShadeArgs a)
{
    using C = TraceShadeCfg<FIRST, EXT, FB, LDS, TAME, CODE>;
    const uint32_t Ppad     = a.screen.pixels_padded;
    // FIRST: the identity queue of the whole batch, chunk = slot * (Ppad / 64) + 64-pixel group.  Otherwise: chunk slots of the
    // input queue.  Either way the grid is persistent (the LDS tables are staged once per workgroup, not once per frame slot).
    const uint32_t cps      = Ppad >> 6;
    const uint32_t chunks   = FIRST ? cps * a.n_slots : (a.in.class_capacity >> 6) * kQueueClasses;
    uint32_t       n_shaded = 0, n_probed = 0;
    __shared__ FrameConst lds_frames[kMaxFrameSlots];
    __shared__ float4     lds_shade[LDS ? kShadeRec * kExhaustiveMax : 1];
    __shared__ float4     lds_rec[LDS ? 4 * kExhaustiveMax : 1];
    __shared__ float4     lds_probe[C::PROBE ? 2 * kMaxFrameSlots : 1];
    __shared__ float      lds_pscore[C::PROBE ? kExhaustiveMax / 2 : 1];
    __shared__ SlotSample lds_first[(C::LEAN && FIRST) ? kMaxFrameSlots : 1];  // bounce 0 only (512 B; bounce >= 1 stays at its 25 732 B)
    __shared__ uint32_t   lds_probe_k;
    __shared__ float4     lds_ring[(C::PROBE && !FIRST) ? (kBlock / 64) * kWaveRing : 1];  // per wave: (origin, path id) of its parked shadow rays
    __shared__ float4     lds_org[C::ORG ? kExhaustiveMax : 1];
    __shared__ float4     lds_bounds[C::ORG ? kExhaustiveMax / 2 : 1];
    __shared__ float      lds_mat[C::XT ? 12 * kExhaustiveMax : 1];
    __shared__ float      lds_lcdf[C::XT ? kExtLightsMax : 1];
    __shared__ float4     lds_lrec[C::XT ? 4 * kExtLightsMax : 1];
    const bool            ext_tabs = C::XT && a.scene.material_count <= kExhaustiveMax && a.scene.light_count <= kExtLightsMax;  // wave-uniform
    if (LDS)
    {
        stage_scene_records(bvh, a, lds_shade, lds_rec);
        if (C::XT && ext_tabs) stage_ext_tables(a, lds_mat, lds_lcdf, lds_lrec);
        if (C::ORG) stage_camera_pairs(bvh, a, lds_org, lds_bounds);
    }
    if (C::PROBE && a.inline_probe) stage_probe_rows(bvh, a, lds_pscore, lds_probe_k, lds_probe);
    if constexpr (C::LEAN)
        stage_frames_samples<FIRST>(a, lds_frames, lds_first);  // ends with the workgroup barrier
    else
        stage_frames(a, lds_frames);  // ends with the workgroup barrier
    ProbeArgs probe;
    if (C::PROBE && a.inline_probe) probe.rows = lds_probe, probe.pairs = bvh.fan_pairs, probe.k = lds_probe_k;
    // The probe's survivors stay with the wave that found them (ShadeArgs::wave_ring): parked in its own 128-entry ring and traced
    // 64 at a time between chunks -- the any-hit kernel's loop on full waves, without its launch, its queue round trip, or any
    // other wave.  No plane entry is shared: within one launch a path either escapes (sky term) or has a vertex (this shadow
    // ray), and the previous bounce's additions were made by the previous launch.
    uint32_t ring_head = 0, ring_n = 0;  // wave-uniform
    if (C::PROBE && !FIRST && a.inline_probe && a.wave_ring)  // (bounce 0: more survivors per chunk, and a kernel short of registers: 2.4 -> 2.9 ms for the 0.35 ms of its any-hit launch)
    {
        probe.ring_org = lds_ring + (threadIdx.x >> 6) * kWaveRing;  // origins + path ids in LDS, the contributions in this wave's
        probe.ring_con = a.shadow.contrib_pid + (size_t)wave_global_id() * kWaveRing;  // slice of the shadow queue's memory
    }
    auto trace_ring = [&](uint32_t count) {
        // The ring is a cross-lane hand-off inside one wave: lane i stored entry `pos` (LDS origin, global contribution), lane j
        // loads it here.  Commit 6a9000f put a scheduling barrier here after reading the ISA, not after a failure: nothing but
        // may-alias analysis kept the compiler from hoisting these loads above the stores of the inlined shade_vertex.  The memory
        // model's statement of the same thing: release after the stores (shade_vertex), acquire before the loads.
        wave_handoff();
        const uint32_t lane_ = threadIdx.x & 63u;
        const bool     on    = lane_ < count;
        const uint32_t pos   = (ring_head + lane_) & (kWaveRing - 1u);
        float4         o     = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) o = probe.ring_org[pos];
        const uint32_t spid = f2u(o.w);
        const bool     good = on && (spid >> kPidShift) < a.n_slots && (spid & kPidMask) < Ppad;
        const FrameConst& fc = lds_frames[good ? (spid >> kPidShift) : 0u];
        const Ray  sr = make_ray(mk3(o.x, o.y, o.z), mk3(fc.light_dir[0], fc.light_dir[1], fc.light_dir[2]), kRayEps, good ? kRayFar : kRayEps);
        // what the probe left over is mostly unoccluded, and the path id came out of LDS: the contribution and the plane entry are
        // requested before the test and arrive under it
        float4* const target = a.bounce == 0 ? a.planes.direct : a.planes.color;
        const size_t  idx    = good ? (size_t)(spid >> kPidShift) * Ppad + (spid & kPidMask) : 0;
        float4        c = make_float4(0.f, 0.f, 0.f, 0.f), cur = c;
        if (good) c = probe.ring_con[pos], cur = target[idx];
        const bool occluded = exhaustive_any<false>(bvh, sr);
        // lighting.h:57-60: unoccluded -> the contribution evaluated at shading time is added
        if (good && !occluded) target[idx] = make_float4(cur.x + c.x, cur.y + c.y, cur.z + c.z, cur.w);
        ring_head = (ring_head + count) & (kWaveRing - 1u);
        ring_n -= count;
    };
    const float4* shade_tab = LDS ? lds_shade : a.scene.shade_tris;
    const float4* rec_tab   = LDS ? lds_rec : bvh.tris_by_id;
    ExtTables     xtabs;
    if (C::XT && ext_tabs) xtabs.materials = reinterpret_cast<const MaterialDev*>(lds_mat), xtabs.light_cdf = lds_lcdf, xtabs.light_rec = lds_lrec;
    Stamps st;
    st.start();
    // Chunk slots from the class's work counter, like the any-hit kernel (with the priorities below: bounce 0 4.6 -> 4.1 ms,
    // bounce >= 1 unchanged; before them it cost the bounce >= 1 kernel 7 %).  As there, the class's length is read once and
    // the next grab is issued after the entry loads (see k_trace_any).
    const uint32_t my_class = wave_global_id() % kQueueClasses;
    const uint32_t lane     = threadIdx.x & 63u;
    uint32_t       n_class  = 0;
    if (!FIRST)
    {
        n_class = a.in.count[my_class * kCounterStride];
        n_class = n_class < a.in.class_capacity ? n_class : a.in.class_capacity;
    }
    uint32_t grab = grab_issue(a.work, my_class);
    while (true)
    {
        const uint32_t j = grab_value(grab);  // slot j of this class
        uint32_t       i, pid = 0, slot = 0;
        const uint32_t klass = my_class;      // the path's class for its whole life
        bool           active;
        v3             thr = mk3(1.0f, 1.0f, 1.0f);
        Ray            r   = make_ray(mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 1.f), 0.0f, 0.0f);  // empty interval: hits nothing
        float          carried_r1 = 0.f, carried_r2 = 0.f;
        if (FIRST)
        {
            const uint32_t chunk = class_chunk(j, my_class);
            if (chunk >= chunks) break;  // (only in or past the last block of 64 chunks: every earlier block holds each class once)
            grab   = grab_issue(a.work, my_class);
            slot   = chunk / cps;  // wave-uniform
            i      = (chunk - slot * cps) * 64 + lane;
            active = true;
            pid    = (slot << kPidShift) | i;
            uint32_t x, y;
            if (local_pixel_to_xy(a.screen, i, x, y))
                r = make_ray(mk3(a.cam.position[0], a.cam.position[1], a.cam.position[2]),
                             primary_dir(a.cam, a.screen, lds_frames[slot], x, y), 0.0f, kPrimaryFar);
        }
        else
        {
            if (j * 64u >= n_class) break;  // past the end of this class's sub-queue
            active = j * 64u + lane < n_class;
            if constexpr (C::LEAN)
            {
                // A lane past the end of the class's last chunk loads the class's LAST entry (n_class > j * 64 >= 0 here, and
                // n_class <= class_capacity: inside the sub-queue) instead of taking defaults that cost a v_mov per register and chunk, and
                // the entry's registers are used where they land.  Such a lane holds a real path's ray and id, but active == false, and
                // that alone keeps it silent: has_ray == false clears its candidate mask (so it hits nothing and reads no record),
                // pre.valid == false makes shade_vertex skip every store, count and emit for it, and the only tables it indexes -- the
                // frame slot's rows -- it indexes with that real, in-range slot.
                const uint32_t local = j * 64u + lane;
                i                    = my_class * a.in.class_capacity + (local < n_class ? local : n_class - 1u);
                const float4 o = a.in.org_tmin[i], d = a.in.dir_tmax[i], tp = a.in.thr_pid[i];
                grab = grab_issue(a.work, my_class);
                r    = make_ray(mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z), kRayEps, kRayFar);
                thr  = mk3(tp.x, tp.y, tp.z), pid = f2u(tp.w);
                carried_r1 = o.w, carried_r2 = d.w;
            }
            else
            {
                i      = my_class * a.in.class_capacity + j * 64u + lane;
                // extension rays: tmin / tmax are constants (rt_indirect.hlsl:154-157); with C::CARRY the .w slots hold the sample
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f), d = make_float4(0.f, 0.f, 1.f, 0.f), tp = make_float4(1.f, 1.f, 1.f, 0.f);
                if (active) o = a.in.org_tmin[i], d = a.in.dir_tmax[i], tp = a.in.thr_pid[i];
                grab = grab_issue(a.work, my_class);
                if (active)
                {
                    r   = make_ray(mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z), kRayEps, kRayFar);
                    thr = mk3(tp.x, tp.y, tp.z), pid = f2u(tp.w);
                    carried_r1 = o.w, carried_r2 = d.w;
                }
            }
        }
        float    t, u, v;
        uint32_t gid;
        STAMP(st, 0, true);  // queue entry arrived
        // The triangle loop is the long, purely arithmetic phase; everything around it (queue reads, shading with its LDS gathers,
        // the append atomic, the stores) is short and latency-bound.  Raising the wave's priority outside the loop lets those
        // phases issue ahead of other waves' loops, so more memory operations are in flight per SIMD (closest 18.1 -> 17.5 ms;
        // the opposite assignment: no gain).
        uint32_t pair_mask = ~0u;
        if (C::ORG)
        {
            // the tile of this chunk against the pairs' screen bounds: lane k answers for pair k
            uint32_t tx = 0, ty = 0;
            (void)local_pixel_to_xy(a.screen, i & ~63u, tx, ty);  // first pixel of the 8x8 tile
            const float4 b    = lds_bounds[lane < kExhaustiveMax / 2 ? lane : 0u];
            const bool   over = lane < bvh.fan_pair_count && b.x < (float)(tx + 8u) && b.z >= (float)tx && b.y < (float)(ty + 8u) && b.w >= (float)ty;
            pair_mask         = (uint32_t)__ballot(over);
        }
        __builtin_amdgcn_s_setprio(0);
#if !defined(CAP_CLOSEST_V1)
        if constexpr (LDS && !C::ORG)
        {
            if (bvh.tri_count > 32u)  // wave-uniform, the same for the whole launch
                exhaustive_closest_marked<true>(bvh, rec_tab, r, active, t, u, v, gid);
            else
                exhaustive_closest_marked<false>(bvh, rec_tab, r, active, t, u, v, gid);
        }
        else
#endif
            exhaustive_closest<C::ORG, !LDS>(bvh, rec_tab, r, t, u, v, gid, lds_org, pair_mask);
        __builtin_amdgcn_s_setprio(3);
        STAMP(st, 1, true);  // triangle loop + winner's record
        const ShadePre pre = shade_prefetch<C>(a, lds_frames, active, pid, carried_r1, carried_r2, lds_first);
        if (FIRST && slot == a.aov_slot)
        {
            // rt_primary_visibility.hlsl:46: (uv, asfloat(InstanceID), asfloat(PrimitiveIndex)); a miss keeps uv = 0, ids = ~0u
            float4 g = make_float4(0.f, 0.f, u2f(kInvalidId), u2f(kInvalidId));
            if (gid != kInvalidId)
            {
                const uint4 id = a.scene.tri_ids[gid];
                g              = make_float4(u, v, u2f(id.x), u2f(id.y));
            }
            a.planes.aov_geo[i] = g;
        }
        if constexpr (EXT)
        {
            if (a.inline_nee)  // wave-uniform
            {
                v3 acc = mk3(0.f, 0.f, 0.f);
                if (!FIRST && active)
                {
                    const float4 q = a.in.acc[i];
                    acc            = mk3(q.x, q.y, q.z);
                }
                shade_vertex_ext<FIRST, true>(a, shade_tab, pre, klass, pid, make_float4(u, v, u2f(gid), t), thr, r.d, n_shaded, &bvh, acc, xtabs);
            }
            else
                shade_vertex_ext<FIRST>(a, shade_tab, pre, klass, pid, make_float4(u, v, u2f(gid), t), thr, r.d, n_shaded, nullptr, mk3(0.f, 0.f, 0.f), xtabs);
        }
        else
        {
            shade_vertex<C>(a, shade_tab, pre, klass, pid, make_float4(u, v, u2f(gid), t), thr, n_shaded, st, probe, &n_probed, ring_head, &ring_n);
            if (C::PROBE && ring_n >= 64u) trace_ring(64u);
        }
        STAMP(st, 4, false);  // stores issued
    }
    if (!FIRST && !EXT && !FB) st.flush();
#ifdef CAP_STAMPS
    if (!FIRST && !EXT && !FB && (threadIdx.x & 63u) == 0 && wave_global_id() < 16384)
    {
        g_wave_times[2 * wave_global_id() + 0] = st.t_begin;
        g_wave_times[2 * wave_global_id() + 1] = __builtin_amdgcn_s_memrealtime();
    }
#endif
    if (C::PROBE && ring_n != 0u) trace_ring(ring_n);  // what is left in this wave's ring
    flush_stats(a.out.count + (size_t)my_class * kCounterStride, n_shaded, n_probed);
}

#ifdef CAP_STAMPS
extern "C" int cap_debug_stamps(unsigned long long* out, int reset)
{
    if (reset == 2) return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_times), 2 * 16384 * sizeof(unsigned long long));
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), 8 * sizeof(unsigned long long));
    if (e == hipSuccess && reset)
    {
        unsigned long long z[16] = {};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z));
    }
    return (int)e;
}
#endif

// cap_debug_get(CAP_DEBUG_SELFTEST_SHADE_UNARY / _DIV2): the unscaled forms of the small-scene shading against the plain sqrtf and `/`
// compiled in the same kernel, bit for bit, over every float of the range each is used on (out[0]: mismatches, out[1]: comparisons made).
//   which 0: sqrt_pos and sqrt_unscaled over every normal x >= 2^-96 (both), sqrt_unscaled at +0, -0 and +inf;
//            1 / sqrt(x) as normalize3_tame computes it over every x in [kNormLo, kNormHi];
//            x / kPi over x = 0 and every x in [2^-80, 2]; over every 0 < x < 2^-80, denormals included, the unscaled quotient must be
//            finite and below 1e-5 (what `pdf < 1e-5f` needs of it);
//            f = (kInvPi x) / (x / kPi) over every x in [0, 2] whose pdf passes !(pdf < 1e-5f).
//   which 1: ortho_vector's sqrt and two quotients over 2^31 pseudo-random (a, b), signs, zeros and -0 included, of which those inside the
//            guard (ortho_in_range, the kernel's own) are compared: the host asks for >= 2^30.
__device__ __forceinline__ uint32_t selftest_hash32(uint32_t x)
{
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}
__global__ __launch_bounds__(kBlock) void k_shade_forms_selftest(unsigned long long* out, uint32_t which)
{
    const uint32_t     tid = blockIdx.x * kBlock + threadIdx.x, total = gridDim.x * kBlock;
    unsigned long long bad = 0, n = 0;
    auto               differ = [](float x, float y) { return f2u(x) != f2u(y) ? 1u : 0u; };
    if (which == 0)
    {
        for (uint64_t b = ((127ull - 96ull) << 23) + tid; b <= 0x7f7fffffull; b += total)
        {
            const float x = u2f((uint32_t)b), s = sqrtf(x);
            bad += differ(sqrt_pos(x), s) + differ(sqrt_unscaled(x), s), n += 2;
        }
        if (tid < 3)
        {
            const float x = tid == 0 ? 0.0f : (tid == 1 ? -0.0f : __builtin_inff());
            bad += differ(sqrt_unscaled(x), sqrtf(x)), ++n;
        }
        for (uint64_t b = (uint64_t)f2u(kNormLo) + tid; b <= f2u(kNormHi); b += total)
        {
            const float x = u2f((uint32_t)b);
            bad += differ(div_unscaled(1.0f, sqrt_pos(x)), 1.0f / sqrtf(x)), ++n;
        }
        for (uint64_t b = tid; b <= f2u(2.0f); b += total)
        {
            const float x = u2f((uint32_t)b), pdf = x / kPi, fast = div_unscaled(x, kPi);
            if (b == 0 || b >= ((127ull - 80ull) << 23))
                bad += differ(fast, pdf);
            else
                bad += (fast < 1e-5f && fast > -1e-5f) ? 0u : 1u;  // (false for NaN and inf)
            ++n;
            if (!(pdf < 1e-5f)) bad += differ(div_unscaled(kInvPi * fmaxf(x, 0.0f), pdf), (kInvPi * fmaxf(x, 0.0f)) / pdf), ++n;
        }
    }
    else
    {
        for (uint64_t i = tid; i < (1ull << 31); i += total)
        {
            const uint32_t h0 = selftest_hash32((uint32_t)i), h1 = selftest_hash32((uint32_t)i ^ 0x9e3779b9u), h2 = selftest_hash32(h0 + h1);
            // exponent fields: the larger operand 2^-45 .. 2^44, the other 0 .. 95 binades below it (both ends beyond the guard)
            const uint32_t e1 = 82u + h2 % 90u, d = (h2 >> 8) % 96u, e0 = e1 > d ? e1 - d : 1u;
            float          p = u2f((e1 << 23) | (h0 & 0x007fffffu) | ((h2 << 3) & 0x80000000u));
            float          q = u2f((e0 << 23) | (h1 & 0x007fffffu) | ((h2 << 2) & 0x80000000u));
            if ((h2 >> 24 & 7u) == 0u) q = (h2 & 0x08000000u) ? 0.0f : -0.0f;
            const bool  sw = (h2 >> 27 & 1u) != 0u;
            const float a = sw ? q : p, b = sw ? p : q, g = fmaf(a, a, b * b);
            if (!ortho_in_range(a, b, g)) continue;
            const float k = sqrtf(g), kf = sqrt_pos(g);
            float       qa, qb;
            div2_unscaled(a, b, kf, qa, qb);
            bad += differ(kf, k) + differ(qa, a / k) + differ(qb, b / k), ++n;
        }
    }
    if (bad) atomicAdd(&out[0], bad);
    atomicAdd(&out[1], n);
}

void launch_shade_forms_selftest(hipStream_t stream, unsigned long long* out_device, uint32_t which)
{
    hipLaunchKernelGGL(k_shade_forms_selftest, dim3(4096), dim3(kBlock), 0, stream, out_device, which);
}

// The thirteen instantiations that exist, each under the tuple it was instantiated with.  Bounce 0 has no feedback form, the two
// models and feedback exclude each other, TAME is the reference model with the scene in LDS and CODE its bounce 0 (TraceShadeCfg).
enum : uint32_t { TS_FIRST = 1, TS_EXT = 2, TS_FB = 4, TS_LDS = 8, TS_TAME = 16, TS_CODE = 32 };
struct TraceShadeKernel
{
    uint32_t is;
    void (*kernel)(BvhDev, ShadeArgs);
};
template <uint32_t IS>
constexpr TraceShadeKernel trace_shade_kernel()
{
    return {IS, k_trace_shade<(IS & TS_FIRST) != 0, (IS & TS_EXT) != 0, (IS & TS_FB) != 0, (IS & TS_LDS) != 0, (IS & TS_TAME) != 0, (IS & TS_CODE) != 0>};
}
constexpr TraceShadeKernel kTraceShadeKernels[13] = {
    trace_shade_kernel<TS_FIRST | TS_LDS | TS_TAME | TS_CODE>(),
    trace_shade_kernel<TS_FIRST | TS_EXT | TS_LDS>(), trace_shade_kernel<TS_FIRST | TS_EXT>(),
    trace_shade_kernel<TS_FIRST | TS_LDS | TS_TAME>(), trace_shade_kernel<TS_FIRST | TS_LDS>(), trace_shade_kernel<TS_FIRST>(),
    trace_shade_kernel<TS_EXT | TS_LDS>(), trace_shade_kernel<TS_EXT>(),
    trace_shade_kernel<TS_FB | TS_LDS>(), trace_shade_kernel<TS_FB>(),
    trace_shade_kernel<TS_LDS | TS_TAME>(), trace_shade_kernel<TS_LDS>(), trace_shade_kernel<0>(),
};

// the unscaled forms: reference model, scene in LDS, tame shading records (-DCAP_SHADE_IEEE keeps the plain sqrtf and `/`
// everywhere for A/B runs: capsaicin_amd/variants/shadeieee.flags)
static bool tame_kernels(const BvhDev& bvh, const SceneDev& scene)
{
#if defined(CAP_SHADE_IEEE)
    return false;
#else
    return bvh.tri_count <= kExhaustiveMax && scene.shade_tame != 0;
#endif
}
bool trace_shade_has_code_form(const BvhDev& bvh, const SceneDev& scene) { return tame_kernels(bvh, scene); }

uint32_t launch_trace_shade(const LaunchCfg& cfg, const BvhDev& bvh, const ShadeArgs& args, bool ext, bool feedback)
{
    const bool first = args.bounce == 0;
    const bool fb    = feedback && !ext && !first;  // (bounce 0 defines the planes' entries: nothing to reuse yet)
    const bool lds   = bvh.tri_count <= kExhaustiveMax;
    const bool tame  = !ext && !fb && tame_kernels(bvh, args.scene);
    const bool code  = first && args.code_in_color != 0u;
    assert(!code || tame);  // the host's condition for code_in_color: reference model and trace_shade_has_code_form()
    const uint32_t is = (first ? TS_FIRST : 0u) | (ext ? TS_EXT : 0u) | (fb ? TS_FB : 0u) | (lds ? TS_LDS : 0u) | (tame ? TS_TAME : 0u) | (code ? TS_CODE : 0u);
    // the queue's persistent grid; bounce 0's queue is the identity queue of the batch, one entry per padded pixel and frame slot
    const uint32_t gx = queue_grid(cfg, first ? args.screen.pixels_padded * args.n_slots : args.max_count);
    const TraceShadeKernel* k = kTraceShadeKernels;
    while (k->is != is && k + 1 < kTraceShadeKernels + 13) ++k;
    assert(k->is == is);  // the table holds every tuple the lines above can derive
    hipLaunchKernelGGL(k->kernel, dim3(gx), dim3(kBlock), 0, cfg.stream, bvh, args);
    // the kernel's own conditions: the marked loop where it calls exhaustive_closest_marked, the carry chain where that takes it
#if defined(CAP_CLOSEST_V1)
    return 0u;
#else
    if (!lds || first) return 0u;
    return (kMarkCarry && bvh.tri_ids_dense) ? (bvh.tri_count > 32u ? 3u : 2u) : 1u;
#endif
}
}  // namespace cap
