#!/usr/bin/env python3
"""Instanced ray queries against the same scene flattened into world space -- not part of bench.py.

    python tools/instance_bench.py [--instances 64,4096] [--side both|inst|flat] [--sets a,b,c] [--reps 20] [--warmup 3]
                                   [--width 1920 --height 1080] [--old-abi]

Object: a free-standing piece of 4 096 triangles merged from parts of tools/make_sponza_class.py (a vase, a column, an arch:
something rays pass beside and through).  Instances: a jittered square grid in the xz plane with random rotations, seeded.  The
flattened scene is every instance's copy of the object transformed on the host (float64, rounded once) and uploaded as one mesh:
64 instances are 262 k triangles, 4 096 instances 16.8 M.
Ray sets of width x height rays, as tools/query_bench.py: a camera rays over the whole field, b cosine-hemisphere rays from their
hits (on the flattened scene), c random rays in the field's box.
One JSON line per measurement, host clock around cap_sync over `reps` calls after `warmup`:
  frame     the rigid-motion frame: cap_instances_set (device descriptors) + cap_sync on the instanced side; on the flattened side
            cap_scene_update_vertices (device) + cap_bvh_refit, and its AUTO build beside it;
  trace     cap_trace_instances / _occlusion against cap_trace_rays / cap_trace_occlusion on the flattened scene, alternating, the
            flattened scene on the binary tree (CAP_NO_WIDE8=1: the instanced walk's bottom level is the binary tree, like for like)
            and on the default wide view; `differ` is the share of rays whose (instance, triangle) is not the flattened scene's;
  memory    device bytes each context holds (hipMemGetInfo around its construction).
--side flat --old-abi runs the flattened side alone with a library built from an earlier commit (CAP_LIB_VARIANT=<name>,
tools/build_variant.sh).  Kernel times come from a run of this tool under `rocprofv3 --kernel-trace --stats` (k_query_inst,
k_instance_setup, k_tlas_level, the radix sort's kernels; k_query_binary on the flattened side)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from query_bench import camera_rays, hemisphere_rays, random_rays  # noqa: E402

NEW = ("cap_instances_set", "cap_instances_readback", "cap_trace_instances", "cap_trace_instances_occlusion")


def make_object():
    """(positions [V, 3] float32, normals, texcoords, indices [I] uint32, one mesh): 1 536 + 1 152 + 1 408 = 4 096 triangles"""
    import make_sponza_class as gen
    p, n, t, f = gen.merge([gen.vase((-0.7, 0.0, 0.0), 32, 24), gen.cylinder((0.7, 0.0, 0.0), 0.2, 1.8, 24, 24, 0.08),
                            gen.arch((0.0, 1.0, 0.0), 0.7, 0.1, 44, 16)])
    assert len(f) == 4096
    return p.astype(np.float32), n.astype(np.float32), t.astype(np.float32), f.astype(np.uint32).reshape(-1)


def rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def make_instances(n, seed, spacing=3.5):
    """(n, 3, 4) float32 object-to-world: a jittered sqrt(n) x sqrt(n) grid in the xz plane, random rotations"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    ix, iz = np.divmod(np.arange(n), side)
    t = np.stack([(ix - side / 2) * spacing, np.zeros(n), (iz - side / 2) * spacing], -1) + rng.uniform(-0.6, 0.6, (n, 3))
    return np.concatenate([rotations(rng, n), t[:, :, None]], 2).astype(np.float32)


def flatten(obj, M):
    P, N, T, I = obj
    A = M.astype(np.float64)
    fp = (np.einsum("nij,vj->nvi", A[:, :, :3], P.astype(np.float64)) + A[:, None, :, 3]).astype(np.float32).reshape(-1, 3)
    fn = np.einsum("nij,vj->nvi", A[:, :, :3], N.astype(np.float64)).astype(np.float32).reshape(-1, 3)
    fi = (I[None, :].astype(np.int64) + (np.arange(len(M)) * len(P))[:, None]).astype(np.uint32).reshape(-1)
    return fp, fn, np.tile(T, (len(M), 1)), fi, np.array([[len(fp), 0, len(fi), 0, 0, 0xFFFFFFFF, 0, 0]], np.uint32)


def timed(call, sync, reps, warmup):
    for _ in range(warmup):
        call()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def alternating(calls, sync, reps, warmup):
    """ms per call of each of `calls`, measured in turns (a, b, a, b, ...), every call waited for"""
    for c in calls:
        for _ in range(warmup):
            c()
    sync()
    ms = [0.0] * len(calls)
    for _ in range(reps):
        for k, c in enumerate(calls):
            t0 = time.perf_counter()
            c()
            sync()
            ms[k] += (time.perf_counter() - t0) * 1e3
    return [m / reps for m in ms]


def main():
    import torch
    from capsaicin_amd import capi
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", default="64,4096")
    ap.add_argument("--side", default="both", choices=("both", "inst", "flat"))
    ap.add_argument("--sets", default="a,b,c")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--old-abi", action="store_true")
    a = ap.parse_args()
    if a.old_abi:
        for name in NEW:
            capi.SYMBOLS.pop(name)
    L = capi.lib()
    dev = torch.device("cuda", 0)
    n_rays = a.width * a.height
    obj = make_object()
    T = len(obj[3]) // 3

    def line(**kw):
        print(json.dumps(kw), flush=True)

    def held(make):
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info(dev)[0]
        r = make()
        r.sync()
        return r, before - torch.cuda.mem_get_info(dev)[0]

    for n in (int(x) for x in a.instances.split(",")):
        rng = np.random.default_rng(7)
        M0, M1 = make_instances(n, 11), make_instances(n, 12)  # two poses: the frame moves every instance
        inst = flat = None
        if a.side in ("both", "inst"):
            def make_inst():
                r = capi.Renderer(0)
                r.upload_scene(obj[0], obj[1], obj[2], obj[3], np.array([[len(obj[0]), 0, len(obj[3]), 0, 0, 0xFFFFFFFF, 0, 0]], np.uint32))
                r.build_bvh()
                r.set_instances(M0)
                return r
            inst, inst_bytes = held(make_inst)
            line(what="memory", side="instanced", instances=n, bytes=int(inst_bytes))
            descs = []
            for M in (M0, M1):
                d = np.zeros(n, capi.INSTANCE_DESC_DTYPE)
                d["transform"], d["mask"] = M.reshape(n, 12), 0xFF
                descs.append(torch.as_tensor(d.view(np.uint8).reshape(n, 64), device=dev))
            torch.cuda.synchronize()
            k = [0]

            def frame_inst():
                k[0] ^= 1
                capi._check(L.cap_instances_set(inst.ctx, descs[k[0]].data_ptr(), n, capi.INSTANCES_DEVICE, None), "cap_instances_set")
                inst.sync()
            ms = timed(frame_inst, inst.sync, a.reps, a.warmup)
            info = inst.set_instances(M0)
            line(what="frame", side="instanced", instances=n, ms=round(ms, 4), tlas_depth=info.tlas_depth, inert=info.inert)
        if a.side in ("both", "flat"):
            f0 = flatten(obj, M0)
            p1 = torch.as_tensor(flatten(obj, M1)[0], device=dev)
            p0 = torch.as_tensor(f0[0], device=dev)

            def make_flat():
                r = capi.Renderer(0)
                r.upload_scene(*f0)
                r.build_bvh()
                return r
            flat, flat_bytes = held(make_flat)
            bi = flat.bvh_info()
            line(what="memory", side="flattened", instances=n, triangles=int(bi.triangle_count), bytes=int(flat_bytes))
            line(what="build", side="flattened", instances=n, triangles=int(bi.triangle_count), ms=round(float(bi.build_ms), 3))
            k = [0]

            def frame_flat():
                k[0] ^= 1
                flat.update_vertices(p1 if k[0] else p0)
                flat.refit_bvh()
            ms = timed(frame_flat, flat.sync, max(5, a.reps if n <= 256 else a.reps // 2), a.warmup)
            flat.update_vertices(p0)
            flat.refit_bvh()
            line(what="frame", side="flattened", instances=n, triangles=int(bi.triangle_count), ms=round(ms, 4))
        # rays over the field
        ext = float(np.abs(M0[:, :, 3]).max()) + 2.0
        eye = np.array([-ext * 1.05, 0.35 * ext + 3.0, -ext * 1.05])
        fwd = -eye / np.linalg.norm(eye)
        right = -np.cross(fwd, (0.0, 1.0, 0.0))
        right /= np.linalg.norm(right)
        cam = dict(position=eye, forward=fwd, right=right, up=np.cross(fwd, right), focal_length=0.024, sensor_x=0.036)
        sets = {"a": camera_rays(cam, a.width, a.height)}
        tracer = flat if flat is not None else None
        if "b" in a.sets and tracer is not None:
            ftris = f0[0][f0[3].astype(np.int64)].reshape(-1, 3, 3)
            sets["b"] = hemisphere_rays(sets["a"], tracer.trace_rays(sets["a"]), ftris, n_rays, 1e-4 * ext, rng)
            del ftris
        if "c" in a.sets:
            sets["c"] = random_rays(np.array([-ext, -1.0, -ext]), np.array([ext, 3.0, ext]), n_rays, rng)
        for s in a.sets.split(","):
            if s not in sets:
                continue
            rays = torch.as_tensor(sets[s], device=dev)
            h_i, h_f = (torch.empty((n_rays, 4), dtype=torch.float32, device=dev) for _ in range(2))
            o_i, o_f = (torch.empty((n_rays,), dtype=torch.int32, device=dev) for _ in range(2))
            g_i = torch.empty((n_rays,), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            for kind in ("closest", "occlusion"):
                calls, names = [], []
                if inst is not None:
                    names.append("instanced")
                    calls.append((lambda: capi._check(L.cap_trace_instances(inst.ctx, rays.data_ptr(), n_rays, h_i.data_ptr(), g_i.data_ptr(), None),
                                                      "cap_trace_instances")) if kind == "closest" else
                                 (lambda: capi._check(L.cap_trace_instances_occlusion(inst.ctx, rays.data_ptr(), n_rays, o_i.data_ptr(), None),
                                                      "cap_trace_instances_occlusion")))
                if flat is not None:
                    names.append("flattened")
                    calls.append((lambda: flat.trace_rays(rays, out=h_f, sync=False)) if kind == "closest" else
                                 (lambda: flat.trace_occlusion(rays, out=o_f, sync=False)))

                def sync_all():
                    for r in (inst, flat):
                        if r is not None:
                            r.sync()
                for no_wide in ((1, 0) if flat is not None else (0,)):
                    if flat is not None:
                        flat.debug_switch("CAP_NO_WIDE8", no_wide)
                    ms = alternating(calls, sync_all, a.reps, a.warmup)
                    extra = {}
                    if inst is not None and flat is not None:
                        if kind == "closest":
                            fid = h_f[:, 3].view(torch.int32).to(torch.int64)
                            miss = fid < 0
                            same = torch.where(miss, g_i < 0, (g_i.to(torch.int64) * T + h_i[:, 3].view(torch.int32).to(torch.int64)) == fid)
                            extra = {"differ": round(float(1.0 - same.double().mean()), 6), "hit_fraction": round(float(1.0 - miss.double().mean()), 4)}
                        else:
                            extra = {"differ": round(float((o_i != o_f).double().mean()), 6), "occluded_fraction": round(float(o_f.double().mean()), 4)}
                    line(what="trace", instances=n, set=s, kind=kind, rays=n_rays, flattened_tree="binary" if no_wide else "wide",
                         **{"ms_" + nm: round(m, 4) for nm, m in zip(names, ms)},
                         **({"ratio": round(ms[0] / ms[1], 3)} if len(ms) == 2 else {}), **extra)
        for r in (inst, flat):
            if r is not None:
                r.close()
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
