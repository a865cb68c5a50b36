#!/usr/bin/env python3
"""Objects (cap_objects_set) against the mask trick for showing different things in different places -- not part of bench.py.

    python tools/object_bench.py [--instances 64,4096] [--sets a,b,c] [--reps 20] [--warmup 3] [--width 1920 --height 1080]

Scene: eight free-standing objects of 4 096 triangles each, parts of tools/make_sponza_class.py (vases, columns, arches, cloths), one
mesh per object, 32 768 triangles in one upload.  Instances: tools/instance_bench.py's jittered grid with random rotations, instance i
showing object i mod 8.
  side "masks"    the workaround: mesh masks 1 << k, each instance's mask the bit of its object; every instance is an instance of the
                  whole scene (the scene's box, the scene's tree) and the mask rejects the other objects' triangles after the test;
  side "objects"  cap_objects_set with one range per mesh and cap_instances_set_ex with the object indices.
Both sides are contexts of one process on the same scene, transforms and rays, measured in turns; `differ` is the share of rays
whose record, instance or occlusion word is not the other side's (the hit sets are the same: it must be 0).
Ray sets of width x height rays, as tools/instance_bench.py: a camera rays over the whole field, b cosine-hemisphere rays from their
hits, c random rays in the field's box.
One JSON line per measurement, host clock around cap_sync over `reps` calls after `warmup`:
  objects   cap_objects_set: its time (CapObjectsInfo::ms, the forest's build) and the table it reports;
  rebuild   cap_bvh_refit and cap_bvh_build with and without the object table (the difference is the forest's rebuild);
  memory    device bytes the forest and its scratch add (hipMemGetInfo around cap_objects_set);
  frame     cap_instances_set(_ex) with device descriptors + cap_sync on either side;
  trace     cap_trace_instances / _occlusion on either side, alternating.
Kernel times come from a run of this tool under `rocprofv3 --kernel-trace --stats` (k_query_inst, k_forest_relocate, the builders')."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from instance_bench import alternating, make_instances, timed  # noqa: E402
from query_bench import camera_rays, random_rays  # noqa: E402

N_OBJECTS = 8


def make_scene():
    """(positions, normals, texcoords, mesh-local indices, meshes [8, 8]) and the (8 * 4096, 3, 3) triangles: every part 2 * 64 * 32"""
    import make_sponza_class as gen
    parts = [gen.vase((0.0, 0.0, 0.0), 64, 32), gen.cylinder((0.0, 0.0, 0.0), 0.2, 1.8, 64, 32, 0.08), gen.arch((0.0, 0.0, 0.0), 0.7, 0.1, 64, 32),
             gen.cloth((-0.6, 1.4, 0.0), 1.2, 1.3, 64, 32, 3.0, 0.5), gen.vase((0.0, 0.3, 0.0), 32, 64), gen.cylinder((0.0, 0.0, 0.0), 0.35, 0.9, 32, 64, 0.3),
             gen.arch((0.0, 0.2, 0.0), 0.5, 0.16, 32, 64, "z"), gen.cloth((-0.5, 1.0, 0.0), 1.0, 0.9, 32, 64, 5.0, 1.5)]
    P, N, T, I, M = [], [], [], [], []
    nv = ni = 0
    for k, (p, n, t, f) in enumerate(parts):
        assert len(f) == 4096
        M.append([len(p), nv, 3 * len(f), ni, k, 0xFFFFFFFF, 0, 0])
        P.append(p), N.append(n), T.append(t), I.append(f.reshape(-1))
        nv, ni = nv + len(p), ni + 3 * len(f)
    P = np.concatenate(P).astype(np.float32)
    tris = np.concatenate([P[m[1] + i.astype(np.int64)].reshape(-1, 3, 3) for m, i in zip(M, I)])
    return (P, np.concatenate(N).astype(np.float32), np.concatenate(T).astype(np.float32), np.concatenate(I).astype(np.uint32),
            np.array(M, np.uint32)), tris


def hemisphere_rays(rays, hits, inst, tris, M, n, eps, rng):
    """query_bench.hemisphere_rays for instanced hits: the normal is the object-space triangle's, turned by the instance's rotation"""
    ids = hits[:, 3].view(np.uint32)
    ok = np.nonzero(ids != 0xFFFFFFFF)[0]
    pick = np.resize(ok[rng.integers(0, len(ok), n)] if len(ok) < n else ok[:n], n)
    g = ids[pick].astype(np.int64)
    p = rays[pick, 0:3] + hits[pick, 0:1] * rays[pick, 4:7]
    nrm = np.cross(tris[g, 1] - tris[g, 0], tris[g, 2] - tris[g, 0]).astype(np.float64)
    nrm = np.einsum("nij,nj->ni", M[inst[pick], :, :3].astype(np.float64), nrm)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= -np.sign((nrm * rays[pick, 4:7]).sum(1, keepdims=True))
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


def main():
    import torch
    from capsaicin_amd import capi
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", default="64,4096")
    ap.add_argument("--sets", default="a,b,c")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    L = capi.lib()
    dev = torch.device("cuda", 0)
    n_rays = a.width * a.height
    arrays, tris = make_scene()
    ranges = np.array([[k, 1] for k in range(N_OBJECTS)], np.uint32)

    def line(**kw):
        print(json.dumps(kw), flush=True)

    def make():
        r = capi.Renderer(0)
        r.upload_scene(*arrays)
        r.build_bvh()
        return r

    masks_side, objects_side = make(), make()
    masks_side.set_instance_masks((1 << np.arange(N_OBJECTS)).astype(np.uint8))
    # the forest: its build, what it holds, what it adds to a refit and to a build
    torch.cuda.synchronize()
    objects_side.sync()
    before = torch.cuda.mem_get_info(dev)[0]
    info = objects_side.set_objects(ranges)
    objects_side.sync()
    line(what="memory", side="objects", triangles=int(info.triangles), bytes=int(before - torch.cuda.mem_get_info(dev)[0]))
    oi = objects_side.objects_info()
    line(what="objects", count=int(info.count), triangles=int(info.triangles), nodes=int(info.nodes), max_depth=int(info.max_depth),
         ms=round(float(info.ms), 3), builders=sorted(set(int(b) for b in oi["builder"])), depths=[int(d) for d in oi["max_depth"]])
    ms_set = timed(lambda: objects_side.set_objects(ranges), objects_side.sync, max(3, a.reps // 4), 1)
    line(what="objects", call="cap_objects_set", ms=round(ms_set, 3))
    P = torch.as_tensor(arrays[0], device=dev)
    for name, r in (("masks", masks_side), ("objects", objects_side)):
        def refit():
            r.update_vertices(P)
            r.refit_bvh()
        line(what="rebuild", call="cap_bvh_refit", side=name, ms=round(timed(refit, r.sync, max(3, a.reps // 4), 1), 3))
        line(what="rebuild", call="cap_bvh_build", side=name, ms=round(timed(r.build_bvh, r.sync, max(3, a.reps // 4), 1), 3))

    for n in (int(x) for x in a.instances.split(",")):
        rng = np.random.default_rng(7)
        M0 = make_instances(n, 11)
        objects = (np.arange(n) % N_OBJECTS).astype(np.uint32)
        d = np.zeros(n, capi.INSTANCE_DESC_DTYPE)
        d["transform"], d["mask"] = M0.reshape(n, 12), 0xFF
        d_objects = torch.as_tensor(d.view(np.uint8).reshape(n, 64), device=dev)
        d["mask"] = 1 << objects
        d_masks = torch.as_tensor(d.view(np.uint8).reshape(n, 64), device=dev)
        o_dev = torch.as_tensor(objects.astype(np.int32), device=dev)
        torch.cuda.synchronize()

        def frame_masks():
            capi._check(L.cap_instances_set(masks_side.ctx, d_masks.data_ptr(), n, capi.INSTANCES_DEVICE, None), "cap_instances_set")
            masks_side.sync()

        def frame_objects():
            capi._check(L.cap_instances_set_ex(objects_side.ctx, d_objects.data_ptr(), o_dev.data_ptr(), n, capi.INSTANCES_DEVICE, None), "cap_instances_set_ex")
            objects_side.sync()

        def sync_all():
            masks_side.sync()
            objects_side.sync()
        ms = alternating([frame_masks, frame_objects], sync_all, a.reps, a.warmup)
        line(what="frame", instances=n, ms_masks=round(ms[0], 4), ms_objects=round(ms[1], 4))
        # rays over the field
        ext = float(np.abs(M0[:, :, 3]).max()) + 2.0
        eye = np.array([-ext * 1.05, 0.35 * ext + 3.0, -ext * 1.05])
        fwd = -eye / np.linalg.norm(eye)
        right = -np.cross(fwd, (0.0, 1.0, 0.0))
        right /= np.linalg.norm(right)
        cam = dict(position=eye, forward=fwd, right=right, up=np.cross(fwd, right), focal_length=0.024, sensor_x=0.036)
        sets = {"a": camera_rays(cam, a.width, a.height)}
        if "b" in a.sets:
            h, gi = objects_side.trace_instances(sets["a"])
            sets["b"] = hemisphere_rays(sets["a"], h, gi, tris, M0, n_rays, 1e-4 * ext, rng)
        if "c" in a.sets:
            sets["c"] = random_rays(np.array([-ext, -1.0, -ext]), np.array([ext, 3.0, ext]), n_rays, rng)
        for s in a.sets.split(","):
            if s not in sets:
                continue
            rays = torch.as_tensor(sets[s], device=dev)
            h_m, h_o = (torch.empty((n_rays, 4), dtype=torch.float32, device=dev) for _ in range(2))
            o_m, o_o, g_m, g_o = (torch.empty((n_rays,), dtype=torch.int32, device=dev) for _ in range(4))
            torch.cuda.synchronize()
            for kind in ("closest", "occlusion"):
                if kind == "closest":
                    calls = [lambda: capi._check(L.cap_trace_instances(masks_side.ctx, rays.data_ptr(), n_rays, h_m.data_ptr(), g_m.data_ptr(), None), "cap_trace_instances"),
                             lambda: capi._check(L.cap_trace_instances(objects_side.ctx, rays.data_ptr(), n_rays, h_o.data_ptr(), g_o.data_ptr(), None), "cap_trace_instances")]
                else:
                    calls = [lambda: capi._check(L.cap_trace_instances_occlusion(masks_side.ctx, rays.data_ptr(), n_rays, o_m.data_ptr(), None), "cap_trace_instances_occlusion"),
                             lambda: capi._check(L.cap_trace_instances_occlusion(objects_side.ctx, rays.data_ptr(), n_rays, o_o.data_ptr(), None), "cap_trace_instances_occlusion")]
                ms = alternating(calls, sync_all, a.reps, a.warmup)
                if kind == "closest":
                    same = (h_m.view(torch.int32) == h_o.view(torch.int32)).all(1) & (g_m == g_o)
                    extra = {"differ": round(float(1.0 - same.double().mean()), 6), "hit_fraction": round(float((g_o >= 0).double().mean()), 4)}
                else:
                    extra = {"differ": round(float((o_m != o_o).double().mean()), 6), "occluded_fraction": round(float(o_o.double().mean()), 4)}
                line(what="trace", instances=n, set=s, kind=kind, rays=n_rays, ms_masks=round(ms[0], 4), ms_objects=round(ms[1], 4),
                     masks_over_objects=round(ms[0] / ms[1], 3), **extra)
        del sets
        torch.cuda.empty_cache()
    masks_side.close()
    objects_side.close()


if __name__ == "__main__":
    main()
