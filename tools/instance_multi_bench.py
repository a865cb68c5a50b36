#!/usr/bin/env python3
"""Multi-hit instanced ray queries against the closest instanced query -- not part of bench.py.

    python tools/instance_multi_bench.py [--instances 64,4096] [--sets a,b,c] [--multi 1,4,16,0] [--reps 20] [--warmup 3]
                                         [--width 1920 --height 1080] [--closest-only]

Object, instance grids and the camera of tools/instance_bench.py.  Ray sets of width x height rays: a camera rays over the whole
field, b cosine-hemisphere rays from their closest hits (the instanced query's, the hit triangle taken to world space with its
instance's transform), c random rays in the field's box.  One JSON line per measurement, host clock around cap_sync, the calls taken in
turns (closest, k = 1, closest, k = 4, ...) over `reps` rounds after `warmup`:
  closest   cap_trace_instances;
  multi     cap_trace_instances_multi at each k of --multi without counts (k = 0: counts only), with `filled`, the mean number of hit
            slots a ray's page holds, and the ratio to the closest query of the same process.
--closest-only measures cap_trace_instances alone and does not touch the new entry point: with CAP_LIB_VARIANT=<name> it runs on a
library built from an earlier commit (tools/build_variant.sh in a checkout of it), the baseline the multi-hit numbers are divided by
when the two are run alternately in one session."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from instance_bench import make_instances, make_object  # noqa: E402
from query_bench import camera_rays, hemisphere_rays, random_rays  # noqa: E402

NEWER = ("cap_trace_instances_multi",)


def hemisphere_from_instanced(rays, hits, inst, M, obj_tris, n, eps, rng):
    """tools/query_bench.py hemisphere_rays from instanced hits: each hit ray's triangle in world space, indexed by the ray"""
    hit = np.flatnonzero(inst >= 0)
    A = M[inst[hit]].astype(np.float64)
    g = hits[hit, 3].view(np.uint32).astype(np.int64)
    world = np.zeros((len(rays), 3, 3), np.float32)
    world[hit] = np.einsum("nij,nvj->nvi", A[:, :, :3], obj_tris[g].astype(np.float64)) + A[:, None, :, 3]
    by_ray = hits.copy()
    ids = by_ray[:, 3].view(np.uint32)
    ids[hit] = hit.astype(np.uint32)
    return hemisphere_rays(rays, by_ray, world, n, eps, rng)


def main():
    import torch
    from capsaicin_amd import capi
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", default="64,4096")
    ap.add_argument("--sets", default="a,b,c")
    ap.add_argument("--multi", default="1,4,16,0")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--closest-only", action="store_true")
    a = ap.parse_args()
    if a.closest_only:
        for name in NEWER:
            capi.SYMBOLS.pop(name, None)
    L = capi.lib()
    dev = torch.device("cuda", 0)
    n_rays = a.width * a.height
    obj = make_object()
    obj_tris = obj[0][obj[3].astype(np.int64)].reshape(-1, 3, 3)
    ks = [] if a.closest_only else [int(x) for x in a.multi.split(",")]
    library = os.environ.get("CAP_LIB_VARIANT") or "tree"

    def line(**kw):
        print(json.dumps(dict(library=library, **kw)), flush=True)

    for n in (int(x) for x in a.instances.split(",")):
        rng = np.random.default_rng(7)
        M0 = make_instances(n, 11)
        r = capi.Renderer(0)
        r.upload_scene(obj[0], obj[1], obj[2], obj[3], np.array([[len(obj[0]), 0, len(obj[3]), 0, 0, 0xFFFFFFFF, 0, 0]], np.uint32))
        r.build_bvh()
        r.set_instances(M0)
        ext = float(np.abs(M0[:, :, 3]).max()) + 2.0
        eye = np.array([-ext * 1.05, 0.35 * ext + 3.0, -ext * 1.05])
        fwd = -eye / np.linalg.norm(eye)
        right = -np.cross(fwd, (0.0, 1.0, 0.0))
        right /= np.linalg.norm(right)
        cam = dict(position=eye, forward=fwd, right=right, up=np.cross(fwd, right), focal_length=0.024, sensor_x=0.036)
        sets = {"a": camera_rays(cam, a.width, a.height)}
        if "b" in a.sets:
            h, i = r.trace_instances(sets["a"])
            sets["b"] = hemisphere_from_instanced(sets["a"], h, i, M0, obj_tris, n_rays, 1e-4 * ext, rng)
        if "c" in a.sets:
            sets["c"] = random_rays(np.array([-ext, -1.0, -ext]), np.array([ext, 3.0, ext]), n_rays, rng)
        k_max = max(ks + [1])
        hits = torch.empty((n_rays, k_max, 4), dtype=torch.float32, device=dev)
        inst = torch.empty((n_rays, k_max), dtype=torch.int32, device=dev)
        cnt = torch.empty((n_rays,), dtype=torch.int32, device=dev)
        for s in a.sets.split(","):
            if s not in sets:
                continue
            rays = torch.as_tensor(sets[s], device=dev)
            torch.cuda.synchronize()

            def closest():
                capi._check(L.cap_trace_instances(r.ctx, rays.data_ptr(), n_rays, hits.data_ptr(), inst.data_ptr(), None), "cap_trace_instances")

            def multi(k):
                capi._check(L.cap_trace_instances_multi(r.ctx, rays.data_ptr(), n_rays, k, hits.data_ptr() if k else None, inst.data_ptr() if k else None,
                                                        None if k else cnt.data_ptr(), 0, None), "cap_trace_instances_multi")

            calls = [closest] + [(lambda k=k: multi(k)) for k in ks]
            for c in calls:
                for _ in range(a.warmup):
                    c()
            r.sync()
            ms = [0.0] * len(calls)
            for _ in range(a.reps):
                for j, c in enumerate(calls):
                    t0 = time.perf_counter()
                    c()
                    r.sync()
                    ms[j] += (time.perf_counter() - t0) * 1e3
            ms = [m / a.reps for m in ms]
            line(what="closest", instances=n, set=s, rays=n_rays, ms=round(ms[0], 4))
            for k, m in zip(ks, ms[1:]):
                multi(k)
                r.sync()
                filled = float((inst.view(-1)[:n_rays * k] >= 0).sum()) / n_rays if k else float(cnt.double().mean())  # (k = 0: the mean count)
                line(what="multi", instances=n, set=s, rays=n_rays, k=k, counts_only=k == 0, ms=round(m, 4), ratio_to_closest=round(m / ms[0], 3),
                     filled=round(filled, 3))
        r.close()
        del sets, hits, inst, cnt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
