#!/usr/bin/env python3
"""Headline benchmark: Mrays/s (primary + extension + shadow rays actually traced) of the HIP wavefront path tracer on
BASELINE.json configs[1]: cornell_box.obj, 1920x1080, 64 spp, depth 8, on N MI355X GPUs of one node.

One "step" = one complete render of that image: 64 frames (frame_count 0..63) through ray generation -> BVH traversal ->
shading/BSDF sampling -> radiance accumulate; for N > 1 the frame is sharded by 8x8 screen tiles (tile t -> rank t % N) and a
step ends with ONE gather of tile radiance to rank 0 (RCCL) + the assembly of the image there.  Total work is fixed as N
grows ("strong" scaling).  Scene, BVH and blue-noise texture are resident in HBM before the timed region.

Prints one JSON line (rank 0) with the bench contract fields.  A plain run sets up, warms up, times the steps and prints it; with
--dump-outputs DIR it first writes what the last timed step computed (the assembled image, the ray counts) as DIR/*.npy.  --full
adds everything else, as separate runs after the timed steps: `roofline` (dominant kernel: closest-hit traversal of extension rays,
timed with HIP events on the render stream in one more step), `stage_ms_per_rank`, `cpu_baseline` (the scalar CPU oracle on the
host cores), the extra lines (other BASELINE configs, post chain, ingestion, shard costs) and the image's sanity check; the keys
of what a run did not measure are null.
"""
import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WIDTH, HEIGHT, SPP, DEPTH = 1920, 1080, 64, 8
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md); 6.3 TB/s is the measured achievable stream rate
HBM_ACHIEVABLE_GBS = 6300.0  # what a streaming kernel reaches on this chip (MI355X_MICROARCH.md, measured: `empirical_stream_peak`)
TREE_SPP = 32  # one batch of the tree-path variant (tools/tree_trace.sh and tree_pmc.sh profile the same)
TREE_FULL_SPP = 128  # BASELINE configs[3]'s own sample count: four such batches
BIG_SCALE, BIG_SPP = 8.0, 8  # big_variant: the hall at 16.8 M triangles, 8 spp
BYTES_CLOSEST, BYTES_ANY, BYTES_VERTEX = 48, 36, 144  # SURVEY.md 8d algorithmic queue-stream bytes per ray / shaded vertex
# vector-instruction issue peak: one wave64 instruction per 2 cycles per SIMD, 1024 SIMDs, 2.4 GHz (MI355X_MICROARCH.md)
VALU_PEAK_WAVE_INSTS_PER_S = 1024 * 2.4e9 / 2.0
def kernel_source_sha():
    """Hash of everything the profiled kernels and the trees they walk are built from -- every .hip / .h / .cpp of csrc and the
    Makefile with its flags (a builder or a layout change moves traversal bytes just as a kernel change does): committed counter
    files are only quoted while it matches."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "capsaicin_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h", ".cpp")) or f == "Makefile":
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()


def build_extra():
    """The EXTRA flags libcapsaicin_hip.so was linked with (capsaicin_amd/build_flags.txt, written by the Makefile): "" for the product
    build.  tools/ab_define.sh and tools/prof_all.sh leave diagnostic builds behind if they are interrupted before their exit trap."""
    try:
        return open(os.path.join(ROOT, "capsaicin_amd", "build_flags.txt")).read().strip().partition("=")[2].strip()
    except OSError:
        return ""


def committed_counters(key):
    """Per-launch HBM bytes / vector instructions of one kernel from the newest profiles/rNN_traffic.json (PMC passes of this very
    command, tools/make_traffic.py; counters cannot be collected from inside the timed process).  None when the kernel sources
    have changed since the passes were taken."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_traffic.json")))
    if not files:
        return None, None
    if build_extra():
        return None, "not quoted: diagnostic build (EXTRA=%s)" % build_extra()
    try:
        tj = json.load(open(files[-1]))
        if tj.get("source_sha256") != kernel_source_sha():
            return None, os.path.relpath(files[-1], ROOT) + " (stale: kernel sources changed since)"
        return tj["kernels"].get(key), os.path.relpath(files[-1], ROOT)
    except Exception:  # a malformed file must not break the bench line
        return None, None


def roofline_object(kernel_name, counters_key, kernel_bytes, launches, kernel_ms, rays, extra=None, quote_counters=True):
    """The `roofline` object of the bench contract for one kernel: achieved = algorithmic bytes per launch / average launch
    duration (HIP events on the render stream).  `bound` names the limiter the counters show; the HBM fraction stays `frac`."""
    avg_ms = kernel_ms / launches
    bytes_per_launch = kernel_bytes / launches
    achieved = bytes_per_launch / (avg_ms * 1e-3) / 1e9
    pmc, src = committed_counters(counters_key) if quote_counters else (None, None)
    traffic = pmc["hbm_bytes_per_launch"] / (avg_ms * 1e-3) / 1e9 if pmc else None
    valu = None
    if pmc and pmc.get("valu_insts_per_launch"):
        valu = {"wave_insts_per_launch": pmc["valu_insts_per_launch"], "peak_wave_insts_per_s": VALU_PEAK_WAVE_INSTS_PER_S,
                "issue_frac": pmc["valu_insts_per_launch"] / (avg_ms * 1e-3) / VALU_PEAK_WAVE_INSTS_PER_S,
                "note": "issue_frac is against one wave64 instruction per 2 cycles and SIMD at an assumed 2.4 GHz -- the rate of the full-rate class "
                        "only (profiles/r06_micro/valu_cost.txt, s_memtime-timed: FMA / mul / add / mov / bitop3 2.1 cycles per SIMD, conversions, "
                        "min / max, selects, compares, shifts and bit-field operations 4.0, transcendentals 8.0; one wave alone: 4.2 / 8.2).  "
                        "valu_busy_frac and issue_cycles_frac are the counter-derived figures at the clock the kernel really ran at"}
        if pmc.get("valu_busy"):
            vb = pmc["valu_busy"]
            valu.update({"valu_busy_frac": vb["valu_busy_frac"], "issue_cycles_frac": vb.get("issue_cycles_frac"),
                         "static_issue_cycles_per_inst": vb.get("static_issue_cycles_per_inst"), "effective_clock_ghz": vb["effective_clock_ghz"],
                         "valu_busy_note": vb["note"]})
    o = {"bound": "valu", "bound_note": "vector-instruction issue (+ exposed latency), not HBM: see `valu` and DESIGN.md 5; "
                                        "achieved / peak / frac are the contract's algorithmic HBM bytes against the 8 TB/s peak",
         "kernel": kernel_name, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
         "traffic": traffic, "traffic_source": src, "valu": valu, "avg_launch_ms": avg_ms, "launches": int(launches),
         "algorithmic_bytes_per_launch": bytes_per_launch, "bytes_per_ray": kernel_bytes / max(1, rays),
         "rays_per_launch": rays / launches, "kernel_mrays_per_s": rays / (kernel_ms * 1e-3) / 1e6}
    if extra:
        o.update(extra)
    return o


def host_cores():
    """The CPU share this process really has: os.cpu_count() is the machine (256 hardware threads on the GPU box), but the box gives
    one GPU's job a cgroup quota (cpu.max: 16 cores' worth) -- 256 threads on it measured 8.7 x one thread in rounds 3 and 4."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(budget_s=12.0):
    """The oracle (kind "port": scalar C++ restatement, BVH mode) on the same scene/camera/depth, 1 frame at a time."""
    from capsaicin_amd import capi
    from oracle import cap_oracle as O
    from oracle import obj_oracle
    bn = capi.load_bluenoise()
    g = obj_oracle.load_geometry(os.path.join(ROOT, "assets", "cornell_box.obj"))
    sc = O.Scene(g["positions"], g["normals"], g["texcoords"], g["indices"], g["meshes"])
    cam = capi.cornell_camera(WIDTH, HEIGHT)
    ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0],
                         cam.sensor_size[1], cam.focal_length)
    cores = host_cores()
    # All cores: frames side by side, each on its own band of threads (the oracle threads a frame over interleaved rows; one
    # frame at a time on 256 threads spent most of its time starting and joining them: 9x over one thread in round 3).
    import concurrent.futures as cf
    side = max(1, min(8, cores // 4))  # frames side by side, each on its own band of threads
    per = max(1, cores // side)

    def one(frame):
        return sum(sc.render_frame(ocam, bn, WIDTH, HEIGHT, frame, DEPTH, flags=O.FLAG_USE_BVH, threads=per)["rays"])

    rays, frames, t0 = 0, 0, time.time()
    with cf.ThreadPoolExecutor(max_workers=side) as pool:
        while True:
            got = list(pool.map(one, range(frames, frames + side)))  # ctypes releases the GIL for the call
            rays += sum(got)
            frames += side
            el = time.time() - t0
            if el > budget_s or frames >= 64:
                break
    # the same tracer on ONE host thread, one frame at half the resolution per axis
    w1, h1 = WIDTH // 2, HEIGHT // 2
    cam1 = capi.cornell_camera(w1, h1)
    ocam1 = O.make_camera(tuple(cam1.position), tuple(cam1.forward), tuple(cam1.right), tuple(cam1.up), cam1.sensor_size[0],
                          cam1.sensor_size[1], cam1.focal_length)
    t1 = time.time()
    r1 = sc.render_frame(ocam1, bn, w1, h1, 0, DEPTH, flags=O.FLAG_USE_BVH, threads=1)
    el1 = time.time() - t1
    v, v1 = rays / el / 1e6, sum(r1["rays"]) / el1 / 1e6
    return {"value": v, "unit": "Mrays/s", "cores": cores, "hardware_threads": os.cpu_count(), "kind": "port",
            "sample": "%d frame(s) of %dx%d depth %d (of the %d spp workload), oracle BVH mode, %d frames side by side x %d threads, %.1f s" %
                      (frames, WIDTH, HEIGHT, DEPTH, SPP, side, per, el),
            "scaling_over_single_thread": v / v1,
            "single_thread": {"value": v1, "unit": "Mrays/s", "cores": 1,
                              "sample": "1 frame of %dx%d depth %d, %.1f s" % (w1, h1, DEPTH, el1)}}


def load_sponza_class(r, rank=0, scale=1.0, tex_size=256):
    """Generates and uploads the procedural textured hall (tools/make_sponza_class.py: 262 k triangles at scale 1, 4.2 M at 4,
    16.8 M at 8) as GeometryStorage arrays -- bit for bit what the native OBJ loader makes of the OBJ the same tool writes
    (tests/test_obj_loader.py) -- and returns its camera."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_sponza_class as gen
    from capsaicin_amd import capi
    pos, nrm, uv, idx, meshes, texs = gen.arrays(scale, tex_size)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    for i, t in enumerate(texs):
        r.upload_texture(i, t)
    return capi.camera_from_config(dict(gen.camera(), sensor_x=0.036), WIDTH, HEIGHT)


def shard_cost(make_renderer, spp, depth, reps=3):
    """The compute side of the 1 -> 8 GPU curve, measured on ONE device: ms per step for shard 0 of N (tiles t = 0 mod N of every
    frame, exactly what rank 0 of N renders -- every rank's share is the same to within a tile row) and the parallel efficiency it
    predicts before a byte is exchanged, T(1) / (N * T(0 of N)).  `make_renderer()` returns a Renderer with scene, tree, camera and
    resolution set."""
    r = make_renderer()
    out = {}
    for n in (1, 2, 4, 8):
        r.set_shard(0, n)
        r.render(0, spp, depth, 0)
        r.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            r.accum_reset()
            r.render(0, spp, depth, 0)
        r.sync()
        out[n] = (time.perf_counter() - t0) / reps * 1e3
    r.close()
    return {"ms_shard0_of_N": {str(n): out[n] for n in out},
            "predicted_parallel_efficiency": {str(n): out[1] / (n * out[n]) for n in out}}

# ---------------------------------------------------------------------------------------------------------------------------
# Extra lines (N = 1): the other BASELINE configs and the frames the north star's roofline target is about.  Each is a function
# of (device index, torch stream handle) that builds its own context, so that `--only NAME` can run one of them alone -- which
# is how tools/prof.sh takes per-workload kernel traces and counter passes (one workload per rocprofv3 run).
# ---------------------------------------------------------------------------------------------------------------------------
def timed(r, frame_begin, spp, depth, flags, reps):
    """reps renders of spp frames each, accumulation reset in between; (seconds per render, stats summed over the reps)."""
    r.sync()
    r.stats_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        r.accum_reset()
        r.render(frame_begin, spp, depth, flags)
    r.sync()
    return (time.perf_counter() - t0) / reps, r.stats()


def check_guards(st, what):
    if st.guard_shade or st.guard_trace_any or st.guard_append:
        raise SystemExit("%s: kernel bounds guards fired: shade=%d trace_any=%d append=%d last=0x%x" %
                         (what, st.guard_shade, st.guard_trace_any, st.guard_append, st.guard_last))


def stage_ms(sp):
    return {"primary": sp.ms_primary, "trace_closest": sp.ms_trace_closest, "trace_any": sp.ms_trace_any, "shade": sp.ms_shade,
            "resolve": sp.ms_resolve, "total": sp.ms_total}


def cornell_ext_materials():
    """cornell_box.mtl's Kd / Ke + the GGX lobes of assets/scene_config.json: the literal "Lambert+GGX ... emissive" scene."""
    import shutil
    import tempfile
    from capsaicin_amd import capi
    tmp = tempfile.mkdtemp(prefix="cornell_mtl_")
    txt = open(os.path.join(ROOT, "assets", "cornell_box.obj")).read().replace("mtllib cornellbox.mtl", "mtllib cornell_box.mtl")
    open(os.path.join(tmp, "c.obj"), "w").write(txt)
    shutil.copy(os.path.join(ROOT, "assets", "cornell_box.mtl"), os.path.join(tmp, "cornell_box.mtl"))
    mats = capi.Geometry(os.path.join(tmp, "c.obj")).materials()
    for m, (rough, ks) in capi.scene_config()["cornell_ggx"].items():
        mats[int(m), 3], mats[int(m), 4:7] = rough, ks
    return mats


def make_cornell(device_index, stream, width=WIDTH, height=HEIGHT, ext=False, shard=(0, 1)):
    from capsaicin_amd import capi
    r = capi.Renderer(device_index, stream)
    r.upload_geometry(capi.Geometry(os.path.join(ROOT, "assets", "cornell_box.obj")))
    r.upload_bluenoise(capi.load_bluenoise())
    r.build_bvh()
    r.set_resolution(width, height)
    r.set_shard(*shard)
    r.set_camera(capi.cornell_camera(width, height))
    if ext:
        r.upload_materials(cornell_ext_materials())
    return r


def make_hall(device_index, stream, scale=1.0):
    from capsaicin_amd import capi
    r = capi.Renderer(device_index, stream)
    cam = load_sponza_class(r, scale=scale)
    r.upload_bluenoise(capi.load_bluenoise())
    bi = r.build_bvh()
    r.set_resolution(WIDTH, HEIGHT)
    r.set_camera(cam)
    return r, bi


def fused_roofline(sp, name, key, ext, quote):
    """k_trace_shade of bounces >= 1.  Reference model: reads one 48-B queue entry (ray 32 + throughput / path id 16) per extension
    ray, writes one 48-B entry per ray it emits and 32 B per shadow ray its own probe does not answer (CapStats::shadow_entries).
    EXT model: 64-B entries (+ the 16 B of radiance the path has gathered), no shadow entries (the next-event ray is traced where
    it is generated)."""
    ext_out = sp.rays_extension - sp.rays_extension_bounce0
    if ext:
        kb = 64 * sp.rays_extension + 64 * ext_out + 48 * (sp.shadow_entries - sp.shadow_entries_bounce0)
    else:
        kb = 48 * sp.rays_extension + 48 * ext_out + 32 * (sp.shadow_entries - sp.shadow_entries_bounce0)
    return roofline_object(name, key, kb, sp.launches_trace_closest, sp.ms_trace_closest, sp.rays_extension, quote_counters=quote), kb


def ext_variant(dev, stream, steps, spp=SPP):
    from capsaicin_amd import capi
    r = make_cornell(dev, stream, ext=True)
    r.render(0, spp, DEPTH, capi.RENDER_EXT_MATERIALS)
    dt, es = timed(r, 0, spp, DEPTH, capi.RENDER_EXT_MATERIALS, steps)
    check_guards(es, "ext_variant")
    _, ep = timed(r, 0, spp, DEPTH, capi.RENDER_EXT_MATERIALS | capi.RENDER_STAGE_TIMERS, 1)
    roof, _ = fused_roofline(ep, "k_trace_shade<bounce>=1, EXT> (exhaustive closest hit + GGX/NEE shading, fused)", "ext", True, spp == SPP)
    r.close()
    erays = es.rays_primary + es.rays_extension + es.rays_shadow
    return {"workload": "cornell_box.obj + cornell_box.mtl %dx%d %dspp depth=%d, Lambert+GGX, emissive lamp + NEE (EXT model)" %
                        (WIDTH, HEIGHT, spp, DEPTH),
            "value": erays / steps / dt / 1e6, "unit": "Mrays/s", "ms_per_step": dt * 1e3,
            "rays_per_step": {"primary": es.rays_primary / steps, "extension": es.rays_extension / steps, "shadow": es.rays_shadow / steps},
            "roofline": roof, "stage_ms": stage_ms(ep)}


def tree_rooflines(tp, key, scene_note, dense=False):
    """The tree path's two priced kernels from one stage-timed render: k_trace_closest8 -- (A) queue bytes, 32-B ray read + 16-B hit
    written, and (A + B) with the nodes and triangle records a ray requests (instrumented build, tools/w8_counts.py,
    committed with the counter passes) -- and k_shade (144 B per shaded vertex; escapes priced separately).
    dense: the scene has >= 2 triangles per pixel, so the camera rays went through k_trace_closest8 as well (context.hip primary_wide):
    one more launch per batch, timed under the primary stage together with the 0.1 ms of k_raygen_identity that feeds it; its rays,
    launches and time are part of the kernel's totals here, as they are of the counter passes' per-dispatch averages."""
    pmc, _ = committed_counters(key)
    trav = pmc.get("traversal_bytes_per_ray") if pmc else None
    k_rays, k_ms, k_launches = tp.rays_extension, tp.ms_trace_closest, tp.launches_trace_closest
    if dense:
        k_rays, k_ms, k_launches = k_rays + tp.rays_primary, k_ms + tp.ms_primary, k_launches + tp.launches_trace_closest // DEPTH
    troof = roofline_object("k_trace_closest8 (%s rays, compressed 8-wide tree)" % ("camera + extension" if dense else "extension"), key,
                            BYTES_CLOSEST * k_rays, k_launches, k_ms, k_rays)
    troof["bound_note"] = scene_note
    if trav:
        ab = (BYTES_CLOSEST + trav) * k_rays / (k_ms * 1e-3) / 1e9
        troof.update({"traversal_bytes_per_ray": trav, "node_steps_per_ray": pmc.get("node_steps_per_ray"),
                      "triangle_tests_per_ray": pmc.get("triangle_tests_per_ray"), "achieved_with_traversal_bytes": ab,
                      "frac_with_traversal_bytes": ab / HBM_PEAK_GBS, "frac_with_traversal_bytes_of_achievable": ab / HBM_ACHIEVABLE_GBS})
    if troof.get("traffic"):
        troof["traffic_frac"] = troof["traffic"] / HBM_PEAK_GBS
        troof["traffic_frac_of_achievable"] = troof["traffic"] / HBM_ACHIEVABLE_GBS
    spmc, ssrc = committed_counters(key + "_shade")
    shade_ms, shade_launches = tp.ms_shade, max(1, tp.launches_shade)
    # bounce 0 is shaded by the camera-ray kernel (k_primary_shade): k_shade sees the vertices of bounces >= 1 -- at least
    # shaded_vertices - rays_primary of them (not every camera ray finds a vertex: a lower bound, on purpose)
    # (dense scenes: bounce 0 has its own k_shade<FIRST> launch, every vertex is k_shade's)
    shade_vertices = tp.shaded_vertices if dense else max(0, tp.shaded_vertices - tp.rays_primary)
    sroof = {"bound": "hbm", "kernel": "k_shade, bounces >= 1 (attributes, material, direct light, BSDF sample, queue compaction)",
             "achieved": BYTES_VERTEX * shade_vertices / (shade_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
             "traffic": (spmc["hbm_bytes_per_launch"] / (shade_ms / shade_launches * 1e-3) / 1e9) if spmc else None,
             "traffic_source": ssrc, "avg_launch_ms": shade_ms / shade_launches, "launches": int(shade_launches),
             "bytes_per_vertex": BYTES_VERTEX, "vertices_per_step": int(shade_vertices)}
    sroof["frac"] = sroof["achieved"] / HBM_PEAK_GBS
    # the escaped extension rays among k_shade's items: 32 B of queue stream (hit 16 + throughput / path id 16) and a 16-B
    # load-add-store of the path's plane entry for the sky term (rt_indirect.hlsl:94-99) each, without being a vertex
    escapes = max(0, int(tp.rays_extension) + (int(tp.rays_primary) if dense else 0) - int(shade_vertices))
    sroof["escapes_per_step"] = escapes
    sroof["achieved_with_escapes"] = (BYTES_VERTEX * shade_vertices + 64 * escapes) / (shade_ms * 1e-3) / 1e9
    sroof["frac_with_escapes"] = sroof["achieved_with_escapes"] / HBM_PEAK_GBS
    return troof, sroof


def tree_variant(dev, stream):
    """BASELINE configs[3] at its own sample count: the 262 k-triangle textured hall, 1920x1080, 128 spp, depth 8 -- two batches of 64
    frame slots, one per lane (the tree path's default of 128 Mi paths per batch, context.hip cap_render).  The stage split and the
    rooflines come from the same render under the stage timers (sub-key batch_64spp: per batch)."""
    from capsaicin_amd import capi
    r2, bi2 = make_hall(dev, stream)
    # warm-up with the batch structure of the timed render (two lanes, 64 frame slots each): a working set that still has to grow
    # inside the timed region costs a fresh 28-GB hipMalloc per lane
    r2.render(0, TREE_FULL_SPP, DEPTH, 0)
    dt, ts = timed(r2, 0, TREE_FULL_SPP, DEPTH, 0, 1)
    check_guards(ts, "tree_variant")
    # Stage split and rooflines: the same two batches, stage-timed, i.e. one after the other on one stream -- what tools/prof.sh
    # profiles (CAP_NO_TWO_LANES=1: a launch's duration is its own), so the per-launch figures of this line, of
    # profiles/rNN_kernel_stats_tree.csv and of the counter passes describe the same launches.
    dts, tp = timed(r2, 0, TREE_FULL_SPP, DEPTH, capi.RENDER_STAGE_TIMERS, 1)
    troof, sroof = tree_rooflines(tp, "tree", "texture-address path + vector-instruction issue + exposed latency (DESIGN.md 5): on this "
                                  "scene the nodes and triangles a ray touches come from L2 / Infinity Cache, not HBM; achieved / frac = "
                                  "queue-stream bytes (A), achieved_with_traversal_bytes = (A + B) requested bytes, traffic = measured HBM bytes")
    r2.close()
    rays = lambda s: s.rays_primary + s.rays_extension + s.rays_shadow
    return {"workload": "sponza_class.obj (procedural, %d triangles, textured) %dx%d %dspp depth=%d, reference shading" %
                        (bi2.triangle_count, WIDTH, HEIGHT, TREE_FULL_SPP, DEPTH),
            "value": rays(ts) / dt / 1e6, "unit": "Mrays/s", "ms_per_step": dt * 1e3,
            "bvh": {"build": "device SAH splits + clustering + 8-wide collapse (cap_bvh_build AUTO)", "depth": int(bi2.max_depth), "build_ms": float(bi2.build_ms)},
            "batch_64spp": {"what": "one batch of 64 frame slots, batches one after the other on one stream (stage timers)",
                            "value": rays(tp) / dts / 1e6, "ms_per_step": dts * 1e3 / 2,
                            "stage_ms": {k: v / 2 for k, v in stage_ms(tp).items()}},
            "roofline": troof, "shade_roofline": sroof}


def big_variant(dev, stream):
    """The frames the north star's roofline target is about: a scene past every cache.  The hall at scale 8 (16.8 M triangles:
    1.07 GB of intersection records, ~0.25 GB of wide nodes, 2.15 GB of shading records against 256 MiB of Infinity Cache), 1920x1080,
    8 spp, depth 8, tree built by cap_bvh_build AUTO on the device."""
    from capsaicin_amd import capi
    t0 = time.perf_counter()
    r, bi = make_hall(dev, stream, scale=BIG_SCALE)
    setup_s = time.perf_counter() - t0
    winfo = r.bvh_wide_info()
    r.render(0, BIG_SPP, DEPTH, 0)
    dt, bs = timed(r, 0, BIG_SPP, DEPTH, 0, 2)
    check_guards(bs, "big_variant")
    # (two whole 8-spp batches, stage-timed: see tree_variant)
    r.set_batch_paths(BIG_SPP * r.tile_buffer_floats() // 4)
    _, bp = timed(r, 0, 2 * BIG_SPP, DEPTH, capi.RENDER_STAGE_TIMERS, 1)
    n_tri_per_pixel = bi.triangle_count / float(WIDTH * HEIGHT)
    troof, sroof = tree_rooflines(bp, "big", "16.8 M triangles: the wide nodes and intersection records no longer fit the Infinity Cache, so "
                                  "`traffic` (measured HBM bytes) approaches the (A + B) bytes a ray requests; frac = (A) alone, "
                                  "frac_with_traversal_bytes = (A + B) against the 8 TB/s peak, traffic_frac = measured bytes against it",
                                  dense=n_tri_per_pixel >= 2.0)
    r.close()
    rays = bs.rays_primary + bs.rays_extension + bs.rays_shadow
    n = int(bi.triangle_count)
    return {"workload": "sponza_class hall at scale %g (procedural, %d triangles, textured) %dx%d %dspp depth=%d, reference shading" %
                        (BIG_SCALE, n, WIDTH, HEIGHT, BIG_SPP, DEPTH),
            "value": rays / 2 / dt / 1e6, "unit": "Mrays/s", "ms_per_step": dt * 1e3,
            "bvh": {"build": "device SAH splits + clustering + 8-wide collapse (cap_bvh_build AUTO)", "depth": int(bi.max_depth), "build_ms": float(bi.build_ms),
                    "wide_nodes": winfo[0], "wide_depth": winfo[1], "triangles_per_s_build": n / (bi.build_ms * 1e-3),
                    "resident_bytes": {"wide_nodes": 80 * winfo[0], "intersection_records": 64 * n, "shading_records": 128 * n}},
            "scene_setup_s": setup_s, "roofline": troof, "shade_roofline": sroof, "stage_ms": {k: v / 2 for k, v in stage_ms(bp).items()},
            # BASELINE.json north_star: ">= 60 % of MI355X HBM-read roofline on BVH-traversal-bound frames".  SURVEY.md 8d defines the
            # achieved figure as (A + B) x rays / time; the measured fabric traffic of the same launches stands beside it (the
            # difference is what L2 serves: the tree's top levels)
            "step_traffic": step_traffic(bp, dt * 1e3),
            "north_star": north_star_object(troof)}


def pattern_ceiling():
    """tools/micro/gather_ceiling.hip on this chip (profiles/r05_micro/gather_ceiling.json): the rate of DEPENDENT scattered fetches of
    80-byte records at the product's packed stride from a 1.3 GB table, in distinct 128-byte lines -- the memory system's ceiling for
    the traversal kernels' access pattern -- and FETCH_SIZE against the known bytes of that pattern (the correction factor)."""
    try:
        rows = json.load(open(os.path.join(ROOT, "profiles", "r05_micro", "gather_ceiling.json")))["rows"]
        r = [x for x in rows if x["mode"] == "lane5p" and x["table_mb"] == 1331 and x["waves_per_simd"] == 6][0]
        return {"tbs": r["tbs_lines128"], "fetch_size_factor": r.get("factor_vs_lines128"), "glines_per_s": r["grecords_per_s"] * r["lines128_per_record"]}
    except Exception:
        return None


def north_star_object(troof):
    """BASELINE.json north_star: ">= 60 % of MI355X HBM-read roofline on BVH-traversal-bound frames".  The headline of this object is
    the MEASURED fabric traffic of the traversal kernel (FETCH_SIZE x the calibrated factor + WRITE_SIZE) over its live launch time
    against the 8 TB/s peak; `met` refers to that figure.  The requested-bytes figure (A + B) is an upper bound that includes what L2
    and the Infinity Cache serve and is NOT what the target is held to."""
    pc = pattern_ceiling()
    frac = troof.get("traffic_frac")
    o = {"target": 0.6, "kernel": "k_trace_closest8", "basis": "measured HBM / fabric traffic of the kernel (rocprofv3 PMC) / live launch time / 8 TB/s",
         "frac_measured_traffic": frac, "met": (frac >= 0.6) if frac is not None else None,
         "measured_traffic_tbs": (troof["traffic"] / 1e3) if troof.get("traffic") else None,
         "pattern_ceiling_tbs": pc["tbs"] if pc else None,
         "pattern_ceiling_note": "tools/micro/gather_ceiling.hip: dependent scattered 80-B record fetches (five 16-B loads per lane, the "
                                 "kernel's node fetch) from a 1.3 GB table, counted in distinct 128-B lines; every fetch shape tried "
                                 "(per-lane 1 / 4 / 5 / 8 pieces, 4- and 8-lane cooperative) reaches the same line rate",
         "frac_of_pattern_ceiling": (troof["traffic"] / 1e3 / pc["tbs"]) if (pc and troof.get("traffic")) else None,
         "fetch_size_factor_scattered": pc["fetch_size_factor"] if pc else None,
         "fetch_size_factor_note": "FETCH_SIZE x this = known bytes of the scattered pattern (one request per distinct 128-B line, tallied "
                                   "at 64 B): the x 2 of MI355X_MICROARCH.md holds for it, tools/make_traffic.py applies 2.0",
         "upper_bound_requested_bytes_A_plus_B_frac": troof.get("frac_with_traversal_bytes"),
         "upper_bound_note": "(A + B) requested bytes include what L2 / Infinity Cache serve: not the figure the target is held to"}
    return o


def step_traffic(sp, ms_per_step):
    """The FRAME's fraction, not one kernel's: measured bytes of every render kernel per step (profiles/rNN_traffic.json `big_step`:
    all kernels' 2 x FETCH_SIZE + WRITE_SIZE per k_trace_closest8 dispatch of the counter run x this step's closest-hit launches)
    over the plain step time."""
    pmc, src = committed_counters("big_step")
    if not pmc or not pmc.get("bytes_per_closest_dispatch"):
        return {"frac": None, "source": src}
    launches = sp.launches_trace_closest / 2 + sp.launches_trace_closest / 2 / DEPTH  # per 8-spp batch: DEPTH extension launches + the camera rays'
    b = pmc["bytes_per_closest_dispatch"] * launches
    return {"bytes_per_step": b, "gbs": b / (ms_per_step * 1e-3) / 1e9, "frac": b / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, "source": src}


def config3_variant(dev, stream):
    """BASELINE configs[2], "the HBM-roofline run": cornell_box 3840x2160, 512 spp, depth 8, EXT model (next-event estimation of
    the emissive lamp), ONE step; the roofline object comes from a stage-timed 64-spp slice of it (four batches of 16 frame slots)."""
    from capsaicin_amd import capi
    w, h, spp = 3840, 2160, 512
    r = make_cornell(dev, stream, w, h, ext=True)
    fl = capi.RENDER_EXT_MATERIALS
    r.render(0, 16, DEPTH, fl)
    dt, st = timed(r, 0, spp, DEPTH, fl, 1)
    check_guards(st, "config3_variant")
    img = r.readback(capi.BUF_ACCUM_SUM)
    import numpy as np
    assert np.isfinite(img).all() and (img[..., 3] == spp).all(), "config3 image is incomplete"
    _, sp = timed(r, 0, 64, DEPTH, fl | capi.RENDER_STAGE_TIMERS, 1)
    roof, _ = fused_roofline(sp, "k_trace_shade<bounce>=1, EXT> at 3840x2160", "config3", True, True)
    r.close()
    rays = st.rays_primary + st.rays_extension + st.rays_shadow
    return {"workload": "cornell_box.obj + cornell_box.mtl %dx%d %dspp depth=%d + next-event estimation (EXT model), 1 step" % (w, h, spp, DEPTH),
            "value": rays / dt / 1e6, "unit": "Mrays/s", "ms_per_step": dt * 1e3,
            "rays_per_step": {"primary": st.rays_primary, "extension": st.rays_extension, "shadow": st.rays_shadow},
            "roofline": roof, "stage_ms_64spp_slice": stage_ms(sp)}


def config5_share(dev, stream):
    """BASELINE configs[4], one rank's share: shard 0 of 8 (tiles t = 0 mod 8) of 4096x4096, 1024 spp, depth 16, mixed Lambert / GGX
    / emissive materials (EXT model), ONE step.  Every rank's share is the same to within a tile row, so 8 x this value is the
    8-GPU number before the frame-end gather (33.5 MB per rank)."""
    from capsaicin_amd import capi
    w = h = 4096
    spp, depth = 1024, 16
    r = make_cornell(dev, stream, w, h, ext=True, shard=(0, 8))
    fl = capi.RENDER_EXT_MATERIALS
    r.render(0, 64, depth, fl)  # one whole batch of 64 frame slots: every buffer at its final size before the timed render
    dt, st = timed(r, 0, spp, depth, fl, 1)
    check_guards(st, "config5_share")
    _, sp = timed(r, 0, 64, depth, fl | capi.RENDER_STAGE_TIMERS, 1)  # one batch of 64 frame slots (what the step's batches are), stage-timed
    roof, _ = fused_roofline(sp, "k_trace_shade<bounce>=1, EXT>, shard 0 of 8 of 4096x4096", "config5", True, True)
    r.close()
    rays = st.rays_primary + st.rays_extension + st.rays_shadow
    return {"workload": "cornell_box.obj + cornell_box.mtl %dx%d %dspp depth=%d, Lambert/GGX/emissive (EXT model), shard 0 of 8, 1 step" %
                        (w, h, spp, depth),
            "value": rays / dt / 1e6, "unit": "Mrays/s (this rank)", "ms_per_step": dt * 1e3,
            "rays_per_step": {"primary": st.rays_primary, "extension": st.rays_extension, "shadow": st.rays_shadow},
            "predicted_8gpu_value_before_gather": 8 * rays / dt / 1e6, "roofline": roof, "stage_ms_64spp_slice": stage_ms(sp)}


def post_chain_variant(dev, stream):
    from capsaicin_amd import capi
    rp = make_cornell(dev, stream)
    camp = capi.cornell_camera(WIDTH, HEIGHT)
    rp.render(0, 1, 2, capi.RENDER_AOV)
    out = {"what": "Gather -> Accumulate -> BlurDisocclusion -> Blur x4 -> Combine -> TAA, ms per %dx%d frame, static camera, "
                   "frames 3..22" % (WIDTH, HEIGHT), "algorithmic_bytes_per_frame": WIDTH * HEIGHT * 16 * 19}
    for name, fast in (("exact", 0), ("fast_weights", 1)):
        ps = capi.PostSettings(fast_weights=fast)
        for f in range(3):
            rp.post_frame(ps, f, camp)
        rp.sync()
        t0 = time.perf_counter()
        for f in range(3, 23):
            rp.post_frame(ps, f, camp)
        rp.sync()
        out[name + "_ms"] = (time.perf_counter() - t0) / 20 * 1e3
    rp.close()
    return out


def realtime_frame_variant(dev, stream):
    """The reference's own operating point (VERDICT r4 missing 2): the shipped viewer renders ONE sample per frame with
    num_diffuse_bounces = 1 and G-buffer feedback on, then runs the reconstruction chain (raytracing_system.cpp:262-317,
    gui_system.h:39, viewer/main.cpp:53-54).  cornell_box 1920x1080, default CapPostSettings, static camera, frames 3..22; ms per
    frame of the ray passes, of the chain and of both, exact and with fast_weights."""
    from capsaicin_amd import capi
    r = make_cornell(dev, stream)
    cam = capi.cornell_camera(WIDTH, HEIGHT)
    fl = capi.RENDER_AOV | capi.RENDER_GBUFFER_FEEDBACK
    out = {"what": "1 spp, num_bounces 1, G-buffer feedback, then Gather -> Accumulate -> BlurDisocclusion -> Blur x4 -> Combine -> TAA; "
                   "cornell_box %dx%d, static camera, frames 3..22, ms per frame" % (WIDTH, HEIGHT)}
    for name, fast in (("exact", 0), ("fast_weights", 1)):
        ps = capi.PostSettings(fast_weights=fast)
        r.post_reset()

        def frame(f):
            r.set_prev_camera(cam)  # static camera: the previous frame's is this one (raytracing_system.cpp:268-276)
            r.render(f, 1, 1, fl)
            r.post_frame(ps, f, cam)

        for f in range(3):
            frame(f)
        r.sync()
        r.stats_reset()
        t0 = time.perf_counter()
        for f in range(3, 23):
            frame(f)
        r.sync()
        total = (time.perf_counter() - t0) / 20 * 1e3
        st = r.stats()
        # GPU time of the two halves (hipEvent spans on the stream); `total` is the wall clock of the loop
        out[name] = {"ms_per_frame": total, "ray_passes_ms": st.ms_total / 20, "chain_ms": st.ms_post / 20,
                     "chain_passes_ms": dict(zip(("gather", "temporal", "eaw", "combine", "taa"), (x / 20 for x in st.ms_post_pass))),
                     "frames_per_s": 1e3 / total, "rays_per_frame": (st.rays_primary + st.rays_extension + st.rays_shadow) / 20}
    # The viewer's real use is a fly camera (input_system.cpp:49-148), not a tripod (VERDICT r5 missing 4): the same loop with the camera
    # moving every frame -- a dolly along the view with a strafe and a slow turn, the per-frame steps of a hand on W + A and the mouse --
    # so that reprojection misses at the silhouettes, BlurDisocclusion has tiles to filter, and IntegrateTemporally / TAA take their
    # moving branches from frame 8 on, where the static loop above stages nothing.
    import math

    def fly(f):
        c = capi.CameraData.from_buffer_copy(bytes(cam))
        yaw = math.radians(180.0 + 0.15 * f)
        fwd = (math.sin(yaw), 0.0, math.cos(yaw))
        c.forward[:] = fwd
        c.right[:] = (-fwd[2], 0.0, fwd[0])  # normalize(-cross(forward, (0, 1, 0))), input_system.cpp:134-141
        c.up[:] = (0.0, 1.0, 0.0)
        c.position[0] = cam.position[0] + 0.004 * f
        c.position[1] = cam.position[1] + 0.001 * f
        c.position[2] = cam.position[2] - 0.012 * f
        return c

    out["moving"] = {"what": "the same loop, camera moving every frame: 12 mm dolly + 4 mm strafe + 0.15 degrees of yaw per frame, frames 3..22"}
    for name, fast in (("exact", 0), ("fast_weights", 1)):
        ps = capi.PostSettings(fast_weights=fast)
        r.post_reset()

        def mframe(f):
            c, p = fly(f), fly(max(0, f - 1))
            r.set_camera(c)
            r.set_prev_camera(p)
            r.render(f, 1, 1, fl)
            r.post_frame(ps, f, p)

        for f in range(3):
            mframe(f)
        r.sync()
        r.stats_reset()
        t0 = time.perf_counter()
        for f in range(3, 23):
            mframe(f)
        r.sync()
        total = (time.perf_counter() - t0) / 20 * 1e3
        st = r.stats()
        out["moving"][name] = {"ms_per_frame": total, "ray_passes_ms": st.ms_total / 20, "chain_ms": st.ms_post / 20,
                               "chain_passes_ms": dict(zip(("gather", "temporal", "eaw", "combine", "taa"), (x / 20 for x in st.ms_post_pass))),
                               "frames_per_s": 1e3 / total, "rays_per_frame": (st.rays_primary + st.rays_extension + st.rays_shadow) / 20}
    r.close()
    return out


def ingest_variant(dev, stream):
    """The step BEFORE the path (asset_load_system.cpp:43-255, texture_system.cpp:38-118): the 262 k-triangle textured
    hall as an OBJ + MTL + twelve 1024 x 1024 texture files on disk (written by tools/make_sponza_class.py, not timed) through the
    product's own ingestion -- cap_obj_load (parse, triangulate, MeshComponent table), cap_image_decode of the texture files on the
    host's threads, cap_scene_upload_geometry + cap_texture_upload (bilinear footprints built on the device), cap_bvh_build."""
    import shutil
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    from capsaicin_amd import capi
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_sponza_class as gen
    tmp = tempfile.mkdtemp(prefix="cap_ingest_")
    try:
        ntri = gen.write(tmp, 1.0, 1024)
        obj = os.path.join(tmp, "sponza_class.obj")
        obj_bytes = os.path.getsize(obj)
        t0 = time.perf_counter()
        geo = capi.Geometry(obj)
        t_parse = time.perf_counter() - t0
        files = [os.path.join(tmp, "textures", os.path.basename(n)) if not os.path.exists(os.path.join(tmp, n)) else os.path.join(tmp, n)
                 for n in geo.texture_names]
        tex_bytes = sum(os.path.getsize(f) for f in files)
        threads = max(1, min(len(files), host_cores()))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:  # ctypes releases the GIL inside cap_image_decode
            texs = list(ex.map(lambda f: capi.image_decode(open(f, "rb").read(), f), files))
        t_decode = time.perf_counter() - t0
        r = capi.Renderer(dev, stream)
        t0 = time.perf_counter()
        r.upload_geometry(geo)
        for i, t in enumerate(texs):
            r.upload_texture(i, t)
        r.sync()
        t_upload = time.perf_counter() - t0
        r.upload_bluenoise(capi.load_bluenoise())
        t0 = time.perf_counter()
        bi = r.build_bvh()
        t_build = time.perf_counter() - t0
        r.close()
        total = t_parse + t_decode + t_upload + t_build
        return {"what": "sponza_class.obj (%d triangles, %.1f MB of OBJ text) + MTL + %d textures of 1024 x 1024 (%.1f MB of files): disk -> traceable scene"
                        % (ntri, obj_bytes / 1e6, len(files), tex_bytes / 1e6),
                "parse_ms": t_parse * 1e3, "parse_mb_per_s": obj_bytes / 1e6 / t_parse, "parse_mtriangles_per_s": ntri / 1e6 / t_parse,
                "texture_decode_ms": t_decode * 1e3, "texture_decode_threads": threads, "texture_decode_mpixels_per_s": len(files) * 1024 * 1024 / 1e6 / t_decode,
                "upload_ms": t_upload * 1e3, "build_ms": float(bi.build_ms), "build_wall_ms": t_build * 1e3,
                "build_mtriangles_per_s": ntri / 1e6 / (bi.build_ms * 1e-3), "total_ms": total * 1e3, "mtriangles_per_s": ntri / 1e6 / total}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def progress(what):
    """A line on stderr per phase: where a run is, should it ever stop (stdout carries the one JSON line only)."""
    print("[bench %7.1f s] %s" % (time.perf_counter() - T_START, what), file=sys.stderr, flush=True)


T_START = time.perf_counter()


def guarded(fn, *a):
    """An extra line must never cost the contract line."""
    progress(getattr(fn, "__name__", "extra"))
    try:
        return fn(*a)
    except SystemExit:
        raise
    except Exception as exc:
        return {"error": "%s: %s" % (type(exc).__name__, exc)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", choices=("cornell", "sponza"), default="cornell",
                    help="cornell: BASELINE configs[1], the contract line (default).  sponza: BASELINE configs[3] -- the 262 k-triangle "
                         "textured hall, 1920x1080, 128 spp -- as the sharded workload of --gpus N (second scaling curve)")
    ap.add_argument("--spp", type=int, default=0, help=argparse.SUPPRESS)  # debugging only; the contract run uses 64 (sponza: 128)
    ap.add_argument("--no-cpu-baseline", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-tree-variant", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-extras", action="store_true", help=argparse.SUPPRESS)  # profiling passes: the contract workload only
    ap.add_argument("--only", default="", help=argparse.SUPPRESS)  # one extra workload alone (tools/prof.sh): ext, tree, big, config3, config5
    ap.add_argument("--batch-paths", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--traversal", type=int, default=0, help=argparse.SUPPRESS)  # 0 auto (contract run), 1 stack, 2 exhaustive
    ap.add_argument("--scene", default="", help=argparse.SUPPRESS)  # old name of --workload
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the roofline step, the CPU baseline and the extra lines (N = 1) and check "
                         "the image; a plain run does the headline only")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy: image (H x W x 4 float32, accumulated radiance "
                         "sum + sample count) and rays_per_step (float64: primary, extension, shadow)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.scene:
        args.workload = args.scene
    sponza = args.workload == "sponza"
    spp = args.spp or (TREE_FULL_SPP if sponza else SPP)
    contract = not sponza and spp == SPP

    import numpy as np
    import torch
    import torch.distributed as dist
    from capsaicin_amd import capi

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node %d for --gpus %d" % (args.gpus, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the renderer has no CPU path")
    # CAP_BENCH_BACKEND=gloo is a rehearsal mode for boxes with fewer GPUs than ranks (ranks share devices, the gather goes
    # through host memory); the contract run uses nccl (= RCCL over xGMI), one GPU per rank.
    backend = os.environ.get("CAP_BENCH_BACKEND", "nccl")
    device_index = local_rank % torch.cuda.device_count() if backend == "gloo" else local_rank
    torch.cuda.set_device(device_index)

    if args.only:
        if world != 1:
            raise SystemExit("--only runs on one GPU")
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            fn = {"ext": lambda d, s: ext_variant(d, s, max(1, args.steps), spp), "tree": tree_variant, "big": big_variant, "config3": config3_variant,
                  "config5": config5_share, "post": post_chain_variant, "realtime": realtime_frame_variant, "ingest": ingest_variant}[args.only]
            print(json.dumps({"only": args.only, "result": fn(device_index, stream.cuda_stream)}), flush=True)
        return

    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    comm_device = "cuda" if backend == "nccl" else "cpu"

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r = capi.Renderer(device_index, stream.cuda_stream)
        scene_name = "cornell_box.obj"
        camera = capi.cornell_camera(WIDTH, HEIGHT)
        if sponza:
            # BASELINE configs[3] (tools/make_sponza_class.py), tree traversal kernels
            camera = load_sponza_class(r, rank)
            scene_name = "sponza_class.obj (procedural, textured)"
        else:
            r.upload_geometry(capi.Geometry(os.path.join(ROOT, "assets", "cornell_box.obj")))
        r.upload_bluenoise(capi.load_bluenoise())
        bvh = r.build_bvh()
        r.set_resolution(WIDTH, HEIGHT)
        r.set_shard(rank, world)
        r.set_camera(camera)
        if args.batch_paths:
            r.set_batch_paths(args.batch_paths)
        r.set_traversal(args.traversal)
        # every rank builds its own copy of the tree: the builders are deterministic (prefix sums, integer atomics), so the copies are the
        # same bytes -- shown per rank for the tree path's workload (tests/test_comm_gpu.py asserts it)
        wide_sha = None
        if sponza and args.full:
            import hashlib
            wn, wsrc, _, _ = r.bvh_wide_readback()
            wide_sha = hashlib.sha1(np.ascontiguousarray(wn).tobytes() + np.ascontiguousarray(wsrc).tobytes()).hexdigest()
        tile_floats = r.tile_buffer_floats()
        tile_buf = torch.zeros(tile_floats, dtype=torch.float32, device="cuda")
        gathered = torch.zeros(tile_floats * world, dtype=torch.float32, device="cuda") if rank == 0 else None
        image = torch.zeros(WIDTH * HEIGHT * 4, dtype=torch.float32, device="cuda") if rank == 0 else None

        # The exchange of the product path: cap_comm_* (capsaicin_hip.h) -- ncclGather of tile radiance + assembly on rank 0, on
        # the render stream, below Python.  The 128-byte RCCL id travels through the process group that also carries the
        # barriers.  Before anything is timed the result of one frame is compared, on rank 0, with the same gather done by
        # torch.distributed; every rank then uses the C-ABI path, or -- if RCCL could not be loaded or the comparison failed --
        # every rank uses torch.distributed, and the JSON line says which.
        exchange = "none" if world == 1 else "torch.distributed.gather"
        if world > 1 and backend == "nccl":
            # Agreement between the ranks travels over a gloo side group, on host memory: it does not queue behind a collective
            # that one rank entered and another did not, which is exactly the situation it has to detect (a rank that
            # raised inside the try skipped dist.gather while its peers waited in it).
            ctl = dist.new_group(backend="gloo")

            def agree(flag):
                t = torch.tensor([1 if flag else 0], dtype=torch.int32)
                dist.all_reduce(t, op=dist.ReduceOp.MIN, group=ctl)
                return bool(t.item())

            def attempt(what, fn):
                try:
                    fn()
                    return True
                except capi.CapError as exc:
                    sys.stderr.write("[bench] rank %d: %s failed: %s\n" % (rank, what, exc))
                    return False

            try:
                ids = [capi.comm_unique_id() if rank == 0 else None]
            except capi.CapError:
                ids = [None]
            dist.broadcast_object_list(ids, src=0)
            use_cap = ids[0] is not None
            # every rank must have its communicator before any rank enters the gather
            use_cap = use_cap and agree(attempt("cap_comm_init_rank", lambda: r.comm_init_rank(ids[0], rank, world)))
            if use_cap:
                # 1. the local render (no collective): agree before anybody enters one
                def local():
                    r.accum_reset()
                    r.render(0, 1, DEPTH, 0)
                    r.sync()
                use_cap = agree(attempt("render", local))
            if use_cap:
                # 2. the C-ABI gather: only queued here; a rank that could not queue it tells the others, who then give their
                #    communicator up without waiting for the stream (cap_comm_abort) instead of hanging in cap_sync
                queued = agree(attempt("cap_comm_gather_frame", r.comm_gather_frame))
                if not queued:
                    attempt("cap_comm_abort", r.comm_abort)
                    use_cap = False
            if use_cap:
                # 3. the same tiles through torch.distributed, compared on rank 0 with what the C ABI assembled
                staged = agree(attempt("cap_resolve_tiles", lambda: (r.resolve_tiles(tile_buf.data_ptr()), r.sync())))
                same = False
                if staged:
                    torch.cuda.synchronize()
                    dist.gather(tile_buf, list(gathered.chunk(world)) if rank == 0 else None, dst=0)
                    if rank == 0:
                        def compare():
                            nonlocal same
                            r.assemble_tiles(gathered.data_ptr(), world, image.data_ptr())
                            r.sync()
                            torch.cuda.synchronize()
                            a = r.comm_readback().reshape(-1)
                            same = bool(np.array_equal(a.view(np.uint32), image.cpu().numpy().view(np.uint32)))
                        attempt("assemble / compare", compare)
                    else:
                        same = True
                use_cap = agree(staged and same)
            if use_cap:
                exchange = "cap_comm_gather_frame (ncclGather, C ABI)"
            elif ids[0] is not None:
                attempt("cap_comm_destroy", r.comm_destroy)

        def step(flags=0):
            r.accum_reset()
            r.render(0, spp, DEPTH, flags)
            if exchange.startswith("cap_comm"):
                r.comm_gather_frame()
                return
            r.resolve_tiles(tile_buf.data_ptr())
            if world > 1:
                # the single data-path collective: tile radiance -> rank 0 over xGMI
                if backend == "nccl":
                    dist.gather(tile_buf, list(gathered.chunk(world)) if rank == 0 else None, dst=0)
                else:
                    r.sync()
                    host = tile_buf.cpu()
                    parts = [torch.zeros_like(host) for _ in range(world)] if rank == 0 else None
                    dist.gather(host, parts, dst=0)
                    if rank == 0:
                        gathered.copy_(torch.cat(parts))
            if rank == 0:
                r.assemble_tiles((gathered if world > 1 else tile_buf).data_ptr(), world, image.data_ptr())

        def fence():
            r.sync()
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()

        for _ in range(args.warmup):
            step()
        fence()
        r.stats_reset()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        fence()
        dt = time.perf_counter() - t0
        st = r.stats()
        check_guards(st, "rank %d" % rank)

        # whole-job numbers: MAX time over ranks, SUM of rays over ranks
        red = torch.tensor([dt], dtype=torch.float64, device=comm_device)
        cnt = torch.tensor([st.rays_primary, st.rays_extension, st.rays_shadow, st.shaded_vertices], dtype=torch.float64, device=comm_device)
        if world > 1:
            dist.all_reduce(red, op=dist.ReduceOp.MAX)
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
        dt = float(red.item())
        rays_p, rays_e, rays_s, verts = (float(x) for x in cnt.tolist())
        rays = rays_p + rays_e + rays_s

        # what the last timed step computed, before anything else renders into the same buffers
        img = None
        if rank == 0 and (args.full or args.dump_outputs):
            img = (r.comm_readback() if exchange.startswith("cap_comm") else image.cpu().numpy()).reshape(HEIGHT, WIDTH, 4)
            if args.full:
                # sanity of the product of the timed region: finite image, every pixel accumulated spp frames
                assert np.isfinite(img).all() and (img[..., 3] == spp).all(), "bench image is incomplete"
        if rank == 0 and args.dump_outputs:
            os.makedirs(args.dump_outputs, exist_ok=True)
            np.save(os.path.join(args.dump_outputs, "image.npy"), np.ascontiguousarray(img, dtype=np.float32))
            np.save(os.path.join(args.dump_outputs, "rays_per_step.npy"), np.array([rays_p, rays_e, rays_s], dtype=np.float64) / args.steps)

        stage_ms_per_rank, wide_sha_per_rank, roofline = None, [wide_sha], None
        if args.full:
            # dominant kernel, timed live with HIP events on the render stream (one extra step with per-kernel event brackets)
            r.stats_reset()
            step(capi.RENDER_STAGE_TIMERS)
            fence()
            sp = r.stats()
            # per-rank stage split of that step (a future SCALE run shows where a rank's time goes as N grows)
            mine = [sp.ms_primary, sp.ms_trace_closest, sp.ms_trace_any, sp.ms_shade, sp.ms_resolve, sp.ms_total]
            per_rank = [None] * world
            if world > 1:
                dist.all_gather_object(per_rank, mine)
            else:
                per_rank = [mine]
            stage_ms_per_rank = [dict(zip(("primary", "trace_closest", "trace_any", "shade", "resolve", "total"), m)) for m in per_rank]
            if world > 1:
                wide_sha_per_rank = [None] * world
                dist.all_gather_object(wide_sha_per_rank, wide_sha)
        if args.full and rank == 0 and sp.launches_trace_closest:
            fused = sp.launches_shade == 0
            SH_ENTRY = 32  # reference-model shadow entry: (origin, path id) + (contribution, -); see DESIGN.md "Data layout"
            quote = contract and world == 1
            if fused:
                roofline, kernel_bytes = fused_roofline(sp, "k_trace_shade<bounce>=1> (exhaustive closest hit + shading, fused)", "headline",
                                                        False, quote)
                # + bounce-0 kernel (3 planes + its queue writes), any-hit (16-B origin read per ray, 16-B contribution read and 12 B
                # added per unoccluded ray: counted as 16 + 12 per ray, an upper bound), resolve (48 B per path)
                all_bytes = kernel_bytes + 48 * sp.rays_extension_bounce0 + SH_ENTRY * sp.shadow_entries_bounce0 + 48 * sp.rays_primary + \
                    (16 + 12) * sp.shadow_entries + 48 * sp.rays_primary
            else:
                roofline = roofline_object("k_trace_closest8", "tree", BYTES_CLOSEST * sp.rays_extension, sp.launches_trace_closest,
                                           sp.ms_trace_closest, sp.rays_extension, quote_counters=False)
                all_bytes = BYTES_CLOSEST * sp.rays_extension + 16 * sp.rays_primary + BYTES_ANY * sp.rays_shadow + BYTES_VERTEX * sp.shaded_vertices
            # the empirical stream peak of this box, measured in the same run (1 GiB float copy, read + write)
            empirical = None
            if world == 1:
                try:
                    src_t = torch.empty(1 << 28, dtype=torch.float32, device="cuda").fill_(1.0)
                    dst_t = torch.empty_like(src_t)
                    dst_t.copy_(src_t)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(5):
                        dst_t.copy_(src_t)
                    e1.record()
                    torch.cuda.synchronize()
                    empirical = 5 * 2 * src_t.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9
                    del src_t, dst_t
                except Exception:
                    empirical = None
            roofline.update({"empirical_stream_peak": empirical,
                             "frac_of_empirical": (roofline["achieved"] / empirical) if empirical else None,
                             "whole_step_queue_stream_gbs": all_bytes / (sp.ms_total * 1e-3) / 1e9,
                             "stage_ms": stage_ms(sp)})

        progress("contract steps timed")
        extras = world == 1 and contract and not args.no_extras and args.full
        s_h = stream.cuda_stream
        out = None
        if rank == 0:
            metric = "Mrays/sec (primary+secondary), cornell_box 1080p 64spp" if not sponza else \
                "Mrays/sec (primary+secondary), sponza_class 1080p %dspp (BASELINE configs[3]; not the contract metric)" % spp
            out = {"metric": metric, "value": rays / dt / 1e6, "unit": "Mrays/s",
                   "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
                   "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                   "config": {"workload": scene_name + " %dx%d %dspp depth=%d (reference shading: Lambert + directional light + sky), "
                                          "tile-sharded over %d GPU(s)" % (WIDTH, HEIGHT, spp, DEPTH, world),
                              "triangles": int(bvh.triangle_count), "bvh_depth": int(bvh.max_depth),
                              "rays_per_step": {"primary": rays_p / args.steps, "extension": rays_e / args.steps, "shadow": rays_s / args.steps},
                              "parallelism": "tiles%d" % world, "exchange": exchange, "wide_tree_sha1_per_rank": wide_sha_per_rank},
                   # BASELINE configs[1] reads "Lambert+GGX": that literal configuration is the EXT model's line below (ext_variant);
                   # `value` is the reference's own shading model on the same scene, camera, resolution, spp and depth
                   "value_literal_config": None,
                   # the north star's roofline target is about traversal-bound frames: big_variant's closest-hit kernel (16.8 M triangles)
                   "north_star_traversal_bound": None,
                   "exchange": exchange, "stage_ms_per_rank": stage_ms_per_rank,
                   "roofline": roofline, "ext_variant": None, "tree_variant": None, "big_variant": None, "config3_variant": None,
                   "config5_share": None, "shard_cost": None, "post_chain": None, "realtime_frame": None, "ingest": None, "cpu_baseline": None}
            if args.full and not (args.no_cpu_baseline or world > 1):  # rank 0, N = 1 only; before the extra lines, so that the line below is complete without them
                progress("cpu_baseline")
                out["cpu_baseline"] = cpu_baseline()

        # The extra lines (N = 1): each fills its key as it finishes.  A watchdog prints the line as far as it has got and ends the
        # process should one of them not return (a GPU call that never completes cannot be interrupted from Python): the contract
        # line, its roofline and the CPU baseline are never lost to an extra.
        import threading
        lock, finished = threading.Lock(), threading.Event()

        def put(key, val):
            with lock:
                if out is not None:
                    out[key] = val
                    if key == "ext_variant" and isinstance(val, dict):
                        out["value_literal_config"] = val.get("value")
                    if key == "big_variant" and isinstance(val, dict):
                        out["north_star_traversal_bound"] = val.get("north_star")

        def watchdog(limit_s):
            if finished.wait(limit_s):
                return
            with lock:
                for k in ("ext_variant", "tree_variant", "big_variant", "config3_variant", "config5_share", "shard_cost", "post_chain", "realtime_frame", "ingest"):
                    if out[k] is None:
                        out[k] = {"error": "watchdog: the extra lines did not finish within %d s; this one had not returned" % limit_s}
                        break
                progress("watchdog: printing the line without the unfinished extras")
                print(json.dumps(out), flush=True)
                os._exit(0)

        if rank == 0 and world == 1 and args.full:
            threading.Thread(target=watchdog, args=(int(os.environ.get("CAP_BENCH_EXTRAS_LIMIT_S", "180")),), daemon=True).start()
        # the literal "Lambert+GGX" of BASELINE configs[1] (EXT model: no reference counterpart)
        if world == 1 and not sponza and not args.no_extras and args.full:
            put("ext_variant", guarded(ext_variant, device_index, s_h, args.steps, spp))
        if extras and not args.no_tree_variant:
            put("tree_variant", guarded(tree_variant, device_index, s_h))
            put("big_variant", guarded(big_variant, device_index, s_h))
        if extras:
            put("config3_variant", guarded(config3_variant, device_index, s_h))
            put("config5_share", guarded(config5_share, device_index, s_h))
        # the compute side of the scaling curve on this one device: extra key, N = 1 only
        if extras and not args.no_tree_variant:
            progress("shard_cost")
            put("shard_cost", guarded(lambda: {"what": "ms per step of shard 0 of N on ONE MI355X (no exchange): the compute side of the 1 -> N curve",
                                               "cornell_64spp": shard_cost(lambda: make_cornell(device_index, s_h), SPP, DEPTH),
                                               "sponza_class_32spp": shard_cost(lambda: make_hall(device_index, s_h)[0], TREE_SPP, DEPTH, reps=2),
                                               # BASELINE configs[3] at its own sample count: a rank's 128 frame slots are ONE batch of four times
                                               # the 32-spp line's launches, so the traversal launches' drain (their longest rays, ~60 us whatever
                                               # the launch holds) weighs a quarter as much
                                               "sponza_class_128spp": shard_cost(lambda: make_hall(device_index, s_h)[0], TREE_FULL_SPP, DEPTH, reps=2)}))
        if extras:
            put("post_chain", guarded(post_chain_variant, device_index, s_h))
            put("realtime_frame", guarded(realtime_frame_variant, device_index, s_h))
            put("ingest", guarded(ingest_variant, device_index, s_h))
        finished.set()
        if rank == 0:
            with lock:
                progress("done")
                print(json.dumps(out), flush=True)
        r.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
