#!/usr/bin/env python3
"""Throughput of the ray queries (cap_trace_rays / cap_trace_occlusion) on caller-supplied rays -- not part of bench.py.

    python tools/query_bench.py [--scenes cornell,hall] [--sets a,b,c] [--reps 20] [--warmup 3] [--width 1920 --height 1080]

Ray sets, each of width x height rays:
  a  camera rays (pinhole through the pixel centres, tmin 0, tmax 1e6);
  b  cosine-hemisphere rays leaving the primary hit points of (a) around the triangles' geometric normals (tmin 1e-4 x scene size,
     tmax inf): the render's bounce-1 workload;
  c  uniformly random rays: origin uniform in the scene box, direction uniform on the sphere, tmax inf.
Kinds: closest (cap_trace_rays), occlusion (cap_trace_occlusion), multi1 / multi4 / multi16 (cap_trace_rays_multi, k = 1 / 4 / 16, no
counts), count (cap_trace_rays_multi, k = 0: hit counts only).  Any kind takes ray flags and instance masks as "+" suffixes and then
runs through the _ex entry points (closest+back, occlusion+half+front, multi4+back, count+front ...):
  +back / +front  CAP_RAY_FLAG_CULL_BACK_FACING / CULL_FRONT_FACING;
  +first          CAP_RAY_FLAG_ACCEPT_FIRST_HIT (closest only);
  +pass           every mesh mask 0x0F, inclusion mask 0x01: a mask table is installed and passes everything, so the filtered kernels
                  run the plain call's traversal -- the ratio to the plain kind is the filter's own cost;
  +half           mesh m has mask 1 << (m & 1), inclusion mask 0x01: every other mesh is invisible;
  +null           options = NULL: the plain call through the _ex entry point.
--old-abi binds only the symbols the plain kinds need, for a library built from a commit before the _ex entry points
(CAP_LIB_VARIANT=<name>, tools/build_variant.sh).
Per scene, set and kind one JSON line: host clock around cap_sync over `reps` back-to-back calls after `warmup`
calls (the renderer on its own stream, rays and output resident on the device).  Kernel times come from a separate run of this tool
under `rocprofv3 --kernel-trace --stats` (k_query_closest8 / k_query_any8 / k_query_multi8; k_query_binary / k_query_binary_multi
for rays handed to the binary tree).
The hall is tools/make_sponza_class.py at scale 1.0 (262 k triangles), written to a temporary directory."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def triangles(geo):
    P = geo.positions.reshape(-1, 3)
    out = []
    for m in geo.meshes:
        fv, ni, fi = int(m[1]), int(m[2]), int(m[3])
        out.append(P[geo.indices[fi:fi + (ni // 3) * 3].astype(np.int64) + fv].reshape(-1, 3, 3))
    return np.concatenate(out).astype(np.float32)


def camera_rays(cam, w, h):
    f, rt, up = (np.array(x, np.float64) for x in (cam["forward"], cam["right"], cam["up"]))
    sx = cam["sensor_x"]
    sy = sx * h / w
    xs = ((np.arange(w) + 0.5) / w - 0.5) * sx
    ys = (0.5 - (np.arange(h) + 0.5) / h) * sy
    d = f[None, None] * cam["focal_length"] + xs[None, :, None] * rt[None, None] + ys[:, None, None] * up[None, None]
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    r = np.zeros((h * w, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = cam["position"], 0.0, d.reshape(-1, 3), 1e6
    return r


def hemisphere_rays(rays, hits, tris, n, eps, rng):
    ids = hits[:, 3].view(np.uint32)
    ok = np.nonzero(ids != 0xFFFFFFFF)[0]
    pick = ok[rng.integers(0, len(ok), n)] if len(ok) < n else ok[:n]
    pick = np.resize(pick, n)
    g = ids[pick].astype(np.int64)
    p = rays[pick, 0:3] + hits[pick, 0:1] * rays[pick, 4:7]
    nrm = np.cross(tris[g, 1] - tris[g, 0], tris[g, 2] - tris[g, 0]).astype(np.float64)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= -np.sign((nrm * rays[pick, 4:7]).sum(1, keepdims=True))
    # cosine-weighted around the normal
    u1, u2 = rng.random(n), rng.random(n)
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    a = np.where(np.abs(nrm[:, 0:1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    t = np.cross(nrm, a)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(nrm, t)
    d = t * (r * np.cos(phi))[:, None] + b * (r * np.sin(phi))[:, None] + nrm * np.sqrt(1 - u1)[:, None]
    out = np.zeros((n, 8), np.float32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = p, eps, d, np.inf
    return out


def random_rays(lo, hi, n, rng):
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = np.zeros((n, 8), np.float32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = o, 0.0, d, np.inf
    return out


def scene(name, tmp):
    from capsaicin_amd import capi
    if name == "cornell":
        geo = capi.Geometry(os.path.join(ROOT, "assets", "cornell_box.obj"))
        c = capi.scene_config()["cornell_camera"]
        f = np.float64(c["forward"]) / np.linalg.norm(c["forward"])
        right = np.float64(c["right"]) if "right" in c else -np.cross(f, (0.0, 1.0, 0.0))
        right /= np.linalg.norm(right)
        up = np.float64(c["up"]) if "up" in c else np.cross(f, right)
        cam = dict(position=c["position"], forward=f, right=right, up=up, focal_length=c["focal_length"], sensor_x=c["sensor_x"])
        return geo, cam
    import make_sponza_class as gen
    gen.write(tmp, 1.0, 128)
    geo = capi.Geometry(os.path.join(tmp, "sponza_class.obj"))
    c = gen.camera()
    f = np.float64(c["forward"]) / np.linalg.norm(c["forward"])
    right = -np.cross(f, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    cam = dict(position=c["position"], forward=f, right=right, up=np.cross(f, right), focal_length=c["focal_length"], sensor_x=0.036)
    return geo, cam


def main():
    import torch
    from capsaicin_amd import capi
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="cornell,hall")
    ap.add_argument("--sets", default="a,b,c")
    ap.add_argument("--kinds", default="closest,occlusion")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--old-abi", action="store_true")
    a = ap.parse_args()
    if a.old_abi:
        for name in ("cap_scene_set_instance_masks", "cap_trace_rays_ex", "cap_trace_occlusion_ex", "cap_trace_rays_multi_ex"):
            capi.SYMBOLS.pop(name)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    n = a.width * a.height
    with tempfile.TemporaryDirectory() as tmp:
        for sc in a.scenes.split(","):
            geo, cam = scene(sc, tmp)
            tris = triangles(geo)
            r = capi.Renderer(0)
            r.upload_geometry(geo)
            info = r.build_bvh()
            lo, hi = np.array(info.bounds_lo), np.array(info.bounds_hi)
            size = float(np.max(hi - lo))
            cam_rays = camera_rays(cam, a.width, a.height)
            sets = {"a": cam_rays}
            if "b" in a.sets:
                sets["b"] = hemisphere_rays(cam_rays, r.trace_rays(cam_rays), tris, n, 1e-4 * size, rng)
            if "c" in a.sets:
                sets["c"] = random_rays(lo, hi, n, rng)
            for s in a.sets.split(","):
                rays = torch.as_tensor(sets[s], device=dev)
                hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
                occ = torch.empty((n,), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                for full_kind in a.kinds.split(","):
                    kind, *mods = full_kind.split("+")
                    unknown = set(mods) - {"back", "front", "first", "pass", "half", "null"}
                    if unknown or ("pass" in mods and "half" in mods):
                        raise SystemExit("kind %s: bad suffixes" % full_kind)
                    opts = None  # CapTraceOptions of the suffixes; with any suffix the call goes through the _ex entry point
                    if mods:
                        import ctypes
                        L = capi.lib()
                        flags = (0x10 if "back" in mods else 0) | (0x20 if "front" in mods else 0) | (0x04 if "first" in mods else 0)
                        masked = "pass" in mods or "half" in mods
                        opts = None if mods == ["null"] else ctypes.byref(capi.TraceOptions(flags, 0x01 if masked else 0))
                        if masked:
                            m = np.arange(len(geo.meshes)) & 1
                            r.set_instance_masks(np.full(len(m), 0x0F, np.uint8) if "pass" in mods else (1 << m).astype(np.uint8))
                    if kind == "closest":
                        call = (lambda: r.trace_rays(rays, out=hits, sync=False)) if not mods else (
                            lambda: capi._check(L.cap_trace_rays_ex(r.ctx, rays.data_ptr(), n, hits.data_ptr(), opts), "cap_trace_rays_ex"))
                    elif kind == "occlusion":
                        call = (lambda: r.trace_occlusion(rays, out=occ, sync=False)) if not mods else (
                            lambda: capi._check(L.cap_trace_occlusion_ex(r.ctx, rays.data_ptr(), n, occ.data_ptr(), opts), "cap_trace_occlusion_ex"))
                    else:  # count (k = 0) and multiK, through the C entry points: the binding would allocate the output per call
                        k = 0 if kind == "count" else int(kind[len("multi"):])
                        page = torch.empty((n, k, 4), dtype=torch.float32, device=dev) if k else None
                        pp, cp = (page.data_ptr(), None) if k else (None, occ.data_ptr())
                        call = (lambda: capi._check(capi.lib().cap_trace_rays_multi(r.ctx, rays.data_ptr(), n, k, pp, cp, 0), "cap_trace_rays_multi")) \
                            if not mods else (lambda: capi._check(L.cap_trace_rays_multi_ex(r.ctx, rays.data_ptr(), n, k, pp, cp, 0, opts),
                                                                  "cap_trace_rays_multi_ex"))
                    for _ in range(a.warmup):
                        call()
                    r.sync()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        call()
                    r.sync()
                    ms = (time.perf_counter() - t0) * 1e3 / a.reps
                    if kind == "closest":
                        extra = {"hit_fraction": round(float((hits[:, 3].view(torch.int32) != -1).float().mean()), 4)}
                    elif kind == "occlusion":
                        extra = {"occluded_fraction": round(float(occ.float().mean()), 4)}
                    elif kind == "count":
                        extra = {"mean_hits": round(float(occ.double().mean()), 3)}
                    else:
                        extra = {"mean_filled": round(float((page[:, :, 3].view(torch.int32) != -1).double().sum(1).mean()), 3)}
                    print(json.dumps({"scene": sc, "triangles": int(info.triangle_count), "set": s, "kind": full_kind, "rays": n,
                                      "ms_per_call": round(ms, 4), "mrays_per_s": round(n / ms / 1e3, 1), **extra}), flush=True)
                    if mods:
                        r.set_instance_masks(None)
            r.close()


if __name__ == "__main__":
    main()
