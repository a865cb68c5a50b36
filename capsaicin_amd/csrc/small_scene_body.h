// small_scene_body.h -- the body of the fused small-scene kernels, included by k_trace_shade, k_trace_shade_tab, k_trace_shade_head and the
// latter two's 32-byte-entry forms k_trace_shade_tab_gray and k_trace_shade_head_gray (small_scene.hip) and by nothing else.  It reads the kernel's arguments `bvh` and `a`, its configuration type C (a TraceShadeCfg) and the
// flags FIRST, EXT, FB, LDS and TAB as names; no include guard, on purpose.  (What belongs to the head kernels alone stands under C::HEAD, what the 32-byte forms change under C::GRAY and in the type C::Thr.)  Text and not a function: wrapped in a device function the thirteen kernels without the sample table no longer
// compile to the instructions they had (tools/isa_compare.py against the commit before the table), which is what lets the switch
// CAP_SAMPLE_TABLE = 0 stand for that commit in a measurement.
    const uint32_t Ppad     = a.screen.pixels_padded;
    // FIRST: the identity queue of the whole batch, chunk = slot * (Ppad / 64) + 64-pixel group.  Otherwise: chunk slots of the
    // input queue.  Either way the grid is persistent (the LDS tables are staged once per workgroup, not once per frame slot).
    const uint32_t cps      = Ppad >> 6;
    const uint32_t chunks   = (FIRST || C::HEAD) ? cps * a.n_slots : (a.in.class_capacity >> 6) * kQueueClasses;
    uint32_t       n_shaded = 0, n_probed = 0;
    uint32_t       head_ext = 0, head_shadow = 0, head_probed = 0, head_shaded = 0;  // HEAD: bounce 0's counts of this wave (wave-uniform)
    __shared__ FrameConst lds_frames[kMaxFrameSlots];
    __shared__ float4     lds_shade[LDS ? kShadeRec * kExhaustiveMax : 1];
    __shared__ float4     lds_rec[LDS ? 4 * kExhaustiveMax : 1];
    __shared__ float4     lds_probe[C::PROBE ? 2 * kMaxFrameSlots : 1];
    __shared__ float      lds_pscore[C::PROBE ? kExhaustiveMax / 2 : 1];
    __shared__ SlotSample lds_first[(C::LEAN && FIRST && !TAB) ? kMaxFrameSlots : 1];  // bounce 0 only (512 B; bounce >= 1 stays at its 25 732 B)
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
        stage_frames_samples<FIRST, TAB>(a, lds_frames, lds_first);  // ends with the workgroup barrier
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
        if constexpr (C::HEAD)
        {
            // A path can have a bounce-0 and a bounce-1 entry in this ring at once, in one trace or in two, in either order.  The rule
            // that keeps them apart: NO TWO RING ENTRIES OF A PATH WRITE THE SAME BYTES.  A bounce-0 entry (spare word = the path's
            // code, never 0) does what k_trace_any does for a CODE batch (store_first_direct): it stores the contribution into
            // `direct` and the word color.w = code + kCodeLit, and loads nothing.  A bounce-1 entry (spare word 0) adds to color.xyz
            // and stores those twelve bytes alone -- it does not carry w through as the other kernels' 16-B store does, so it can
            // neither lose the bounce-0 entry's word nor be lost to it.  Both follow, in this wave's issue order, the head's own
            // 16-B store of (0, 0, 0, code).
            if (good && !occluded)
            {
                if (f2u(c.w) != 0u)
                {
                    a.planes.direct[idx] = make_float4(c.x, c.y, c.z, 0.0f);
                    reinterpret_cast<float*>(a.planes.color + idx)[3] = c.w + kCodeLit;
                }
                else
                {
                    float* const t3 = reinterpret_cast<float*>(a.planes.color + idx);
                    t3[0] = cur.x + c.x, t3[1] = cur.y + c.y, t3[2] = cur.z + c.z;
                }
            }
        }
        else if (good && !occluded) target[idx] = make_float4(cur.x + c.x, cur.y + c.y, cur.z + c.z, cur.w);
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
    const uint32_t wave_class = wave_global_id() % kQueueClasses;
    // (HEAD: as a scalar, so that what the loop derives from it once -- sub-queue bases, counter lines -- occupies no vector registers)
    const uint32_t my_class = C::HEAD ? (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_class) : wave_class;
    const uint32_t lane     = threadIdx.x & 63u;
    uint32_t       n_class  = 0;
    if (!FIRST && !C::HEAD)
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
        typename C::Thr thr = thr_of<typename C::Thr>(1.0f, 1.0f, 1.0f);  // (GRAY: one float, see TraceShadeCfg)
        Ray            r   = make_ray(mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 1.f), 0.0f, 0.0f);  // empty interval: hits nothing
        float          carried_r1 = 0.f, carried_r2 = 0.f;
        if constexpr (C::HEAD)
        {
            // Bounce 0 of this chunk's 64 paths, from the camera vertex of their jitter group (k_camera_vertices: a.in.org_tmin =
            // (p, code), a.in.dir_tmax = (n, -) per (group, padded pixel); the slot's group sits in its frame constants' pad1) and the
            // slot's bounce-0 sample terms (a.in.thr_pid = that block of the table): shade_vertex<FIRST, CODE>'s own operations on the
            // same operands.  What that kernel wrote into the extension queue stays in registers: r, thr, pid.
            const uint32_t chunk = class_chunk(j, my_class);  // chunks and classes as FIRST deals them out
            if (chunk >= chunks) break;
            // which (slot, 64-pixel group) the dealt index stands for: the slots of a jitter group back to back (cap_device.h head_chunk,
            // a bijection: the class stays my_class = chunk_class(chunk), so the sub-queues' static capacity holds as it did).  Wave-uniform.
            uint32_t group64;
            head_chunk(a.walk, cps, (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk), slot, group64);
            i    = group64 * 64 + lane;
            pid  = (slot << kPidShift) | i;
            const FrameConst& fc = lds_frames[slot];
            const size_t      at = (size_t)f2u(fc.pad1) * Ppad + i;
            const float4      cp = a.in.org_tmin[at], cn = a.in.dir_tmax[at];
            // the position in the 64 x 64 blue-noise period as shade_prefetch derives it at bounce >= 1
            const uint32_t gt   = __umul24(i >> 6, a.screen.shard_count) + a.screen.shard_index;
            const uint32_t ty   = tile_div(gt, a.screen.tiles_x_mul, a.screen.tiles_x_shift);
            const uint32_t tx   = gt + (ty & 7u) * ((0u - a.screen.tiles_x) & 7u);
            const uint32_t base = ((ty & 7u) << 9) | ((i & 0x38u) << 3) | ((tx & 7u) << 3) | (i & 7u);
            const float4   q0   = a.in.thr_pid[(slot << 12) | base];
            grab = grab_issue(a.work, my_class);
            const v3 L = mk3(fc.light_dir[0], fc.light_dir[1], fc.light_dir[2]);
            const v3 I = mk3(fc.light_intensity[0], fc.light_intensity[1], fc.light_intensity[2]);
            // the plane's entry: (0, 0, 0, code) whatever the code says -- padding, sky, kd or black
            a.planes.color[(size_t)slot * Ppad + i] = make_float4(0.f, 0.f, 0.f, cp.w);
            // SKYP: and the sky plane's, +0 for every lane that stores a code -- padding and sky pixels included, and before the `continue`
            // of a wave without rays -- so that the resolve finds the previous batch's value nowhere.  A lane whose own path escapes at
            // bounce 1 stores its throughput over this zero further down (shade_vertex): same lane, same address, program order, which
            // is what the ring's 12-byte stores rest on too (trace_ring).
            if constexpr (C::SKYP) a.planes.sky[(size_t)slot * Ppad + i] = 0.0f;
            const bool vtx = cp.w == kCodeKd || cp.w == kCodeBlack, lit = cp.w == kCodeKd;
            const v3   p = mk3(cp.x, cp.y, cp.z), n = mk3(cn.x, cn.y, cn.z);
            bool       emit_shadow = false, emit_ext = false;
            v3         dir = unread3(), contrib = unread3();
            float      f = unread_f();
            if (lit)
            {
                const float kd  = a.scene.kd_untextured;
                const float ndl = fmaxf(0.0f, dot3(n, L));
                const v3    c   = mk3(((I.x * kd) * kInvPi) * ndl, ((I.y * kd) * kInvPi) * ndl, ((I.z * kd) * kInvPi) * ndl);
                if (c.x != 0.0f || c.y != 0.0f || c.z != 0.0f) emit_shadow = true, contrib = c;
                dir = hemisphere_dir_tame(n, [&] { return HemiTerms{q0.x, q0.y, q0.z}; });
                const float ndd = dot3(n, dir);
                const float pdf = div_unscaled(fmaxf(0.0f, ndd), kPi);
                if (!(pdf < 1e-5f))
                {
                    f        = 1.0f * div_unscaled(kInvPi * fmaxf(ndd, 0.0f), pdf);  // thr = (1, 1, 1) * f
                    emit_ext = true;  // (num_bounces >= 1, no low-resolution indirect: the host's condition for this form)
                }
            }
            const bool occluded0 = pair_occludes_pre(make_ray(p, L, kRayEps, kRayFar), probe.pairs, probe.k, probe.rows[2u * slot], probe.rows[2u * slot + 1u]);
            const bool probed0   = emit_shadow && occluded0;
            emit_shadow          = emit_shadow && !occluded0;
            const unsigned long long ms = __ballot(emit_shadow);
            head_shaded += (uint32_t)__popcll(__ballot(vtx)), head_probed += (uint32_t)__popcll(__ballot(probed0));
            head_ext += (uint32_t)__popcll(__ballot(emit_ext)), head_shadow += (uint32_t)__popcll(ms);
            // the survivors into the wave's ring, marked by the code in the spare word (trace_ring)
            if (emit_shadow)
            {
                const uint32_t pos  = (ring_head + ring_n + (uint32_t)__popcll(ms & ((1ull << lane) - 1ull))) & (kWaveRing - 1u);
                probe.ring_org[pos] = make_float4(p.x, p.y, p.z, u2f(pid));
                probe.ring_con[pos] = make_float4(contrib.x, contrib.y, contrib.z, kCodeKd);
            }
            ring_n += (uint32_t)__popcll(ms);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            if (ring_n >= 64u) trace_ring(64u);  // room for the 64 entries bounce 1 may park
            active = emit_ext;
            if (__ballot(active) == 0ull) continue;  // no lane of the wave has a ray: no loop, nothing to shade
            r   = make_ray(p, dir, kRayEps, kRayFar);
            thr = thr_of<typename C::Thr>(f, f, f);
        }
        else if (FIRST)
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
                if constexpr (C::GRAY)
                {
                    // the 32-byte entry: (o.xyz, thr) (d.xyz, asfloat(pid)); a lane past the end loads the last entry from these two arrays
                    const float4 o = a.in.org_tmin[i], d = a.in.dir_tmax[i];
                    grab = grab_issue(a.work, my_class);
                    r    = make_ray(mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z), kRayEps, kRayFar);
                    thr  = thr_of<typename C::Thr>(o.w, o.w, o.w), pid = f2u(d.w);
                }
                else
                {
                    const float4 o = a.in.org_tmin[i], d = a.in.dir_tmax[i], tp = a.in.thr_pid[i];
                    grab = grab_issue(a.work, my_class);
                    r    = make_ray(mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z), kRayEps, kRayFar);
                    thr  = thr_of<typename C::Thr>(tp.x, tp.y, tp.z), pid = f2u(tp.w);
                    if (!TAB) carried_r1 = o.w, carried_r2 = d.w;  // (TAB: the constants kRayEps / kRayFar again, not read)
                }
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
                    thr = thr_of<typename C::Thr>(tp.x, tp.y, tp.z), pid = f2u(tp.w);
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
                shade_vertex_ext<FIRST, true>(a, shade_tab, pre, klass, pid, make_float4(u, v, u2f(gid), t), thr3(thr), r.d, n_shaded, &bvh, acc, xtabs);
            }
            else
                shade_vertex_ext<FIRST>(a, shade_tab, pre, klass, pid, make_float4(u, v, u2f(gid), t), thr3(thr), r.d, n_shaded, nullptr, mk3(0.f, 0.f, 0.f), xtabs);
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
    if constexpr (C::HEAD)
    {
        // bounce 0's own counter line of this class (a.in.count: the words its launch and its appends would have counted into) --
        // extension and shadow entries in words 0 and 1, probed and shaded in 2 and 3, each pair one atomic per wave
        unsigned long long* const line0 = reinterpret_cast<unsigned long long*>(a.in.count + (size_t)my_class * kCounterStride);
        if (lane == 0u && (head_ext | head_shadow)) atomicAdd(line0, ((unsigned long long)head_shadow << 32) | (unsigned long long)head_ext);
        if (lane == 0u && (head_probed | head_shaded)) atomicAdd(line0 + 1, ((unsigned long long)head_shaded << 32) | (unsigned long long)head_probed);
    }
