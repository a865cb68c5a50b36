#!/usr/bin/env python3
"""Vertex update + refit (cap_scene_update_vertices / cap_bvh_refit) against a rebuild -- not part of bench.py.

    python tools/refit_bench.py [--scenes cornell,hall,hall16m] [--reps 20] [--warmup 3] [--rays 1048576]

Scenes: the Cornell box, tools/make_sponza_class.py arrays() at scale 1.0 (262 k triangles) and 8.0 (16.8 M).  Animation per frame
f: every vertex moves along y by 0.05 sin(0.7 x + 0.3 z + 0.1 f) (scene units, ~1 % of the hall's height), and mesh 3 is translated
by (0.3 sin(0.1 f), 0.1, 0.2) on top.  Per scene one JSON line:
  update_refit_ms  host clock of update_vertices (device source, a torch tensor) + refit_bvh, around cap_sync, mean of `reps` calls
                   after `warmup` (the positions of the frame are resident on the device before the clock starts);
  refit_ms         CapRefitInfo::ms of the same calls (the refit alone);
  build_ms         host clock of build_bvh (AUTO) on the same scene, same protocol, and CapBvhInfo::build_ms of the last build;
  visits           expected node visits after 1, 10 and 60 animated frames (refit) and of a fresh build of frame 60;
  query_ms         cap_trace_rays on `rays` uniformly random rays (origin in the scene box, tmax inf): refitted tree of frame 60
                   against a fresh build of frame 60.
Kernel times come from a separate run of this tool under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from capsaicin_amd import capi  # noqa: E402


def scene(name):
    if name == "cornell":
        g = capi.Geometry(os.path.join(ROOT, "assets", "cornell_box.obj"))
        return g.positions.reshape(-1, 3), g.normals.reshape(-1, 3), g.texcoords.reshape(-1, 2), g.indices, g.meshes
    import make_sponza_class as gen
    P, N, T, I, D, _ = gen.arrays(1.0 if name == "hall" else 8.0, tex_size=128)
    return P, N, T, I, D


def animate(torch, P0, vmesh, f, mesh=3):
    P = P0.clone()
    P[:, 1] += 0.05 * torch.sin(0.7 * P0[:, 0] + 0.3 * P0[:, 2] + 0.1 * f)
    sel = vmesh == mesh
    P[sel] += torch.tensor([0.3 * np.sin(0.1 * f), 0.1, 0.2], dtype=P.dtype, device=P.device)
    return P


def random_rays(torch, P, n, dev):
    g = torch.Generator(device=dev).manual_seed(5)
    lo, hi = P.min(0).values, P.max(0).values
    o = lo + (hi - lo) * torch.rand((n, 3), device=dev, generator=g)
    d = torch.randn((n, 3), device=dev, generator=g)
    d /= d.norm(dim=1, keepdim=True)
    r = torch.zeros((n, 8), device=dev)
    r[:, 0:3], r[:, 4:7], r[:, 7] = o, d, float("inf")
    return r


def timed(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn(-1)
    sync()
    out = []
    for k in range(reps):
        t = time.perf_counter()
        fn(k)
        sync()
        out.append(1e3 * (time.perf_counter() - t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,hall,hall16m")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    for name in a.scenes.split(","):
        P, N, T, I, D = scene(name)
        r = capi.Renderer(0)
        r.upload_scene(P, N, T, I, D)
        bi = r.build_bvh()
        vmesh = np.zeros(len(P), np.int64)
        for m, d in enumerate(np.asarray(D).reshape(-1, 8)):
            vmesh[int(d[1]):int(d[1]) + int(d[0])] = m
        P0 = torch.as_tensor(np.ascontiguousarray(P, np.float32), device=dev)
        vm = torch.as_tensor(vmesh, device=dev)
        frames = [animate(torch, P0, vm, f) for f in range(3)]
        torch.cuda.synchronize(dev)
        infos = []

        def step(k):
            r.update_vertices(positions=frames[k % 3])
            infos.append(r.refit_bvh())

        upd = timed(step, a.reps, a.warmup, r.sync)
        refit_ms = [i.ms for i in infos[a.warmup:]]
        builds = timed(lambda k: r.build_bvh(), max(3, a.reps // 4), 1, r.sync)
        build_ms = r.bvh_info().build_ms
        # tree quality over an animation, starting from a build of frame 0
        r.update_vertices(positions=animate(torch, P0, vm, 0))
        r.build_bvh()
        visits = {}
        for f in range(1, 61):
            r.update_vertices(positions=animate(torch, P0, vm, f))
            info = r.refit_bvh()
            if f in (1, 10, 60):
                visits["frame%d" % f] = info.expected_node_visits
        visits["built_frame0"] = info.expected_node_visits_built
        P60 = animate(torch, P0, vm, 60)
        f60 = capi.Renderer(0)
        f60.upload_scene(P60.cpu().numpy(), N, T, I, D)
        f60.build_bvh()
        f60.update_vertices(positions=P60)
        visits["fresh_frame60"] = f60.refit_bvh().expected_node_visits  # (an identity refit: the metric of the fresh build)
        rays = random_rays(torch, P60, a.rays, dev)
        hits = torch.empty((a.rays, 4), device=dev)
        torch.cuda.synchronize(dev)
        q = {}
        for key, ctx in (("refit", r), ("fresh", f60)):
            ms = timed(lambda k: ctx.trace_rays(rays, hits, sync=False), 10, 2, ctx.sync)
            q[key] = float(np.mean(ms))
        print(json.dumps({"scene": name, "triangles": int(bi.triangle_count), "update_refit_ms": round(float(np.mean(upd)), 3),
                          "update_refit_ms_min": round(float(np.min(upd)), 3), "refit_ms": round(float(np.mean(refit_ms)), 3),
                          "build_ms_host": round(float(np.mean(builds)), 3), "build_ms": round(build_ms, 3),
                          "ratio_build_over_update_refit": round(float(np.mean(builds)) / float(np.mean(upd)), 2),
                          "visits": {k: round(v, 3) for k, v in visits.items()},
                          "query_ms": {k: round(v, 3) for k, v in q.items()}, "rays": a.rays}), flush=True)
        f60.close()
        r.close()


if __name__ == "__main__":
    main()
