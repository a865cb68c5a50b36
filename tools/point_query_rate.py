#!/usr/bin/env python3
"""Throughput of the closest-point queries (cap_closest_points, cap_signed_distance, cap_closest_points_multi, cap_closest_instances,
cap_closest_instances_multi, cap_signed_distance_instances), of the box overlap queries (cap_overlap_boxes, cap_overlap_instances), of cap_overlap_triangles and cap_overlap_triangles_instances and of cap_winding_numbers and cap_winding_instances on the 262 k-triangle hall -- not part of
bench.py, no pass mark.

    python tools/point_query_rate.py [--points 1048576] [--reps 10] [--warmup 2] [--radius inf | --radius-frac F] [--offset 1e-3]
                                     [--k K [--counts]] [--instances N] [--signed] [--winding [--beta B]]  (--winding goes with --instances N)
                                     [--sweeps [--instances N]]

--winding runs cap_winding_numbers at --beta B (default 2; inf sums every triangle exactly: use fewer --points) after
cap_winding_build, on the same point sets (the radius is not read).  Each line carries its rate, mean_visits = the mean numbers of
dipole terms and of exact triangle terms per point, inside (the share of points with w >= 1/2), and the table build:
table_build_ms beside the tree's bvh_build_ms, and the table's statistics.

--instances N together with --winding runs cap_winding_instances on the --instances layout and the same point sets.  Each line carries
its rate, mean_visits = the means of the four visit counts (far terms at the top level, instances entered, far terms below instances,
exact triangles), inside, derived_build_ms = the host time of building the derived tables (per-instance records, top-level dipoles) and
waiting for them, and as the scale cap_winding_numbers on the same points at the same beta in the same process (flat_ms,
flat_mpoints_per_s, flat_mean_visits, ratio_to_flat = the instanced rate over the flat one; N = 1 is the identity alone).

--signed runs cap_signed_distance after cap_pseudonormals_build.  Each line carries its rate and, measured in the same process on the
same points, cap_closest_points as the baseline (flat_ms, flat_mpoints_per_s, time_over_flat = the signed call's time over the plain
one's), same_records (the share of records equal to the plain call's: has to be 1.0), negative (the share of hits with a negative
distance), and the table build: table_build_ms beside the tree's bvh_build_ms, and the weld's statistics.

--instances N runs cap_closest_instances on the hall under N transforms: instance 0 is the identity, the others stand on a square grid
around it, 1.1 scene sizes apart, each turned about the vertical by an angle of its own (N = 1: the identity alone).  The point sets
are the flat query's, in and around instance 0; each line carries the instanced rate and, as its baseline, cap_closest_points on the
same points in the same process (flat_ms, flat_mpoints_per_s) and the ratio of the two rates.

--instances N together with --signed runs cap_signed_distance_instances on the same layout and point sets after
cap_pseudonormals_build.  Each line carries, measured in the same process on the same points: cap_closest_instances (unsigned_ms,
unsigned_mpoints_per_s, time_over_unsigned = the signed call's time over it), cap_closest_points (flat_ms: for the points whose winner
is instance 0, the identity, it is the flat walk from the same p' on the same object, so extra_over_flat = (ms - unsigned_ms) / flat_ms
says what the second phase costs in flat walks), same_records (the share of points whose record and instance equal
cap_closest_instances': has to be 1.0), in_identity (the share of points whose winner is instance 0) and negative (the share of hits
with a negative distance).

--instances N together with --k K [--counts] runs cap_closest_instances_multi on the same layout and point sets.  Each line carries,
measured in the same process on the same points: (a) cap_closest_points_multi at the same k and counts (flat_ms, flat_mpoints_per_s,
ratio_to_flat), (b) cap_closest_instances (single_ms, single_mpoints_per_s, ratio_to_single), and same_as_flat: the share of equal
pages among the points no neighbour reaches -- those whose listed instances are all 0, the identity; flat_comparable is their share of
all points.  A page without a neighbour's pair holds the flat query's candidates alone, so same_as_flat has to be 1.0.

--k K runs cap_closest_points_multi with pages of K records on the same point sets (--counts: with the candidate counts, which turns
off pruning by the k-th distance; K = 0 needs it); the line then also carries k, counts and mean_candidates -- the mean of the counts,
or without --counts the mean number of records listed per point (at most K).  `hits` and `mean_dist` are those of slot 0.  Without
--k the tool runs cap_closest_points as before.  --radius-frac F sets the radius to F x the scene's size.

--boxes runs cap_overlap_boxes on cubes of half-extent --extent E x the scene's size (default 0.005) around the same point sets, pages
of --k K ids (default 4; --counts: with the candidate counts, which cost the walk nothing): mboxes_per_s, mean_candidates and the share
of empty boxes.  Beside it, measured in the same process, the nearest existing workload: cap_closest_points_multi with counts at the
same K on the same centres, at the radius that gives the same mean candidate count (found by bisection: closest_multi_counts_*).
--boxes together with --instances N runs cap_overlap_instances on the --instances layout with the same cubes as world boxes:
mboxes_per_s, mean_candidates (pairs per box) and the share of empty boxes, and from the same process the flat cap_overlap_boxes rate
on the same boxes (flat_ms, flat_mboxes_per_s, flat_mean_candidates, ratio_to_flat).

--triangles runs cap_overlap_triangles on one query triangle per point: vertices uniform in the cube of edge --extent E x the scene's
size (default 0.005) around the point, so its edges are about E x the scene's size -- pages of --k K ids (default 4; --counts as for --boxes):
mtriangles_per_s, mean_candidates and the share of empty queries.  Beside it, measured in the same process, cap_overlap_boxes on the
bounding boxes of the same triangles (boxes_ms, mboxes_per_s, boxes_mean_candidates) and ratio_to_boxes = triangle rate / box rate.
--triangles together with --instances N runs cap_overlap_triangles_instances on the --instances layout with the same triangles as world
queries: mtriangles_per_s, mean_pairs and the share of empty queries, and from the same process the flat cap_overlap_triangles rate on
the same queries (flat_ms, flat_mtriangles_per_s, flat_mean_candidates, ratio_to_flat = the instanced rate over the flat one) and
cap_overlap_instances on the triangles' bounding boxes (boxes_ms, mboxes_per_s, boxes_mean_pairs, ratio_to_boxes).

--sweeps [--radius R | --radius-frac F] runs cap_sweep_spheres: one sweep per point of the same point sets towards a fixed pseudo-random
unit direction, tmax inf, radius R (default 0.01 x the scene's size): msweeps_per_s, the share of misses and of start overlaps, and
from the same process cap_trace_rays on the same origins and directions as the yardstick (rays_ms, mrays_per_s, ray_misses,
ratio_to_rays = the sweep rate over the ray rate).
--sweeps together with --instances N runs cap_sweep_instances on the --instances layout with the same sweeps as world sweeps:
msweeps_per_s, the share of misses, of start overlaps and of winners in instance 0, and from the same process (a) cap_sweep_spheres on
the same sweeps (scene_ms, scene_msweeps_per_s, ratio_to_scene), (b) cap_sweep_instances over ONE identity instance (identity_ms,
identity_msweeps_per_s, identity_to_scene = its rate over the scene form's: the cost of the instanced walk by itself;
identity_same_as_scene: its records equal the scene form's bit for bit) and (c) cap_closest_instances on the origins (closest_ms,
closest_mpoints_per_s, ratio_to_closest).

Point sets, each of --points points (rounded down to a cube for the grid):
  grid      a regular grid through the scene's box, in raster order (x fastest);
  shuffled  the same points in random order;
  surface   points displaced by up to --offset x the scene's size off random points of random triangles.
For scale, cap_trace_rays on the same number of uniformly random rays (origin in the box, direction on the sphere, tmax inf).
One JSON line per set: host clock around cap_sync over `reps` back-to-back calls after `warmup` calls, the renderer on a stream of its
own, points and records resident on the device; M points (rays) per second.  `hits` is the share of queries that found a triangle,
`mean_dist` the mean distance of those in units of the scene's size.  The hall is tools/make_sponza_class.py at scale 1.0."""
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


def timed(r, call, reps, warmup):
    for _ in range(warmup):
        call()
    r.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    r.sync()
    return (time.perf_counter() - t0) / reps


def hall_transforms(count, lo, hi, rng):
    """(count, 3, 4) float32: the identity, then copies on a square grid in the ground plane around it, 1.1 scene sizes apart, each
    turned about the vertical (y) through its own centre"""
    size = float((hi - lo).max())
    c = 0.5 * (lo + hi)
    M = np.zeros((count, 3, 4), np.float64)
    M[:, :, :3] = np.eye(3)
    side = int(np.ceil(np.sqrt(count)))
    for i in range(1, count):
        a = rng.uniform(0.0, 2.0 * np.pi)
        R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        shift = np.array([(i % side) * 1.1 * size, 0.0, (i // side) * 1.1 * size])
        M[i, :, :3], M[i, :, 3] = R, c + shift - R @ c
    return M.astype(np.float32)


def main():
    import torch
    from capsaicin_amd import capi
    from query_bench import random_rays, scene, triangles
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radius", type=float, default=float("inf"))
    ap.add_argument("--radius-frac", type=float, default=None)
    ap.add_argument("--offset", type=float, default=1e-3)
    ap.add_argument("--k", type=int, default=None)
    ap.add_argument("--counts", action="store_true")
    ap.add_argument("--instances", type=int, default=None)
    ap.add_argument("--signed", action="store_true")
    ap.add_argument("--winding", action="store_true")
    ap.add_argument("--beta", type=float, default=2.0)
    ap.add_argument("--boxes", action="store_true")
    ap.add_argument("--extent", type=float, default=0.005)
    ap.add_argument("--triangles", action="store_true")
    ap.add_argument("--sweeps", action="store_true")
    a = ap.parse_args()
    if a.sweeps and (a.winding or a.signed or a.boxes or a.triangles or a.k is not None):
        ap.error("--sweeps goes with --radius, --radius-frac and --instances only")
    if a.sweeps and a.radius == float("inf") and a.radius_frac is None:
        a.radius_frac = 0.01
    if a.boxes and (a.winding or a.signed):
        ap.error("--boxes goes with --k, --counts, --extent and --instances only")
    if a.triangles and (a.winding or a.signed or a.boxes):
        ap.error("--triangles goes with --k, --counts, --extent and --instances only")
    if (a.boxes or a.triangles) and a.k is None:
        a.k = 4  # (before `out` below is sized: the comparison run writes pages of k records into it)
    if a.winding and (a.signed or a.k is not None):
        ap.error("--winding goes alone or with --instances N: the winding number takes no sign table or pages")
    if a.signed and a.k is not None:
        ap.error("--signed does not go with --k: the sign is defined for the single record")
    if a.instances is not None and a.instances < 1:
        ap.error("--instances N needs N >= 1")
    inst_multi = a.instances is not None and a.k is not None and not a.boxes and not a.triangles
    inst_signed = a.instances is not None and a.signed
    rng = np.random.default_rng(2026)
    dev = torch.device("cuda", 0)
    L = capi.lib()
    with tempfile.TemporaryDirectory() as tmp:
        geo, _ = scene("hall", tmp)
        tris = triangles(geo)
        r = capi.Renderer(0)
        r.upload_geometry(geo)
        info = r.build_bvh()
    lo, hi = np.float64(list(info.bounds_lo)), np.float64(list(info.bounds_hi))
    size = float((hi - lo).max())
    if a.radius_frac is not None:
        a.radius = a.radius_frac * size
    if a.counts and a.k is None and not a.boxes and not a.triangles:
        ap.error("--counts needs --k")
    side = int(round(a.points ** (1.0 / 3.0)))
    while side ** 3 > a.points:
        side -= 1
    n = side ** 3
    ax = [np.linspace(lo[k], hi[k], side) for k in range(3)]
    grid = np.stack(np.meshgrid(ax[2], ax[1], ax[0], indexing="ij"), -1).reshape(-1, 3)[:, ::-1]  # x fastest
    g = rng.integers(0, len(tris), n)
    b = rng.dirichlet((1, 1, 1), n)
    surface = np.einsum("nk,nkj->nj", b, tris[g].astype(np.float64)) + (rng.random((n, 3)) - 0.5) * 2 * a.offset * size
    sets = (("grid", grid), ("shuffled", grid[rng.permutation(n)]), ("surface", surface))
    out = torch.empty((n * max(a.k or 1, 1), 8), dtype=torch.float32, device=dev)
    if a.instances is not None:
        M = hall_transforms(a.instances, lo, hi, np.random.default_rng(2027))  # (a generator of its own: the point sets stay the flat runs')
        info_i = r.set_instances(M)
        inst = torch.empty((n * max(a.k or 1, 1),), dtype=torch.int32, device=dev)
        flat_out = torch.empty((n * max(a.k or 1, 1), 8), dtype=torch.float32, device=dev)
        single_out, flat_cnt = (torch.empty((n, 8), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)) if inst_multi else (None, None)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev) if a.counts else None
    if a.signed:
        pn = r.build_pseudonormals()
        signed = torch.empty((n,), dtype=torch.float32, device=dev)
        flat_out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        plain_inst = torch.empty((n,), dtype=torch.int32, device=dev) if inst_signed else None
    head = dict(scene="hall", triangles=int(info.triangle_count), depth=int(info.max_depth), n=n, radius=a.radius, reps=a.reps)
    if a.winding:
        wn = r.build_winding()
        w = torch.empty((n,), dtype=torch.float32, device=dev)
        visits = torch.empty((n, 2), dtype=torch.int32, device=dev)
        if a.instances is not None:
            visits4 = torch.empty((n, 4), dtype=torch.int32, device=dev)
            r.sync()
            t0 = time.perf_counter()
            capi._check(L.cap_winding_instances_readback(r.ctx, None, None, None), "cap_winding_instances_readback")  # builds, and waits
            derived_ms = (time.perf_counter() - t0) * 1e3
            wi = r.winding_instances_info()
        for name, xyz in sets:
            q = np.zeros((n, 4), np.float32)
            q[:, 0:3] = xyz
            pts = torch.as_tensor(q, device=dev).contiguous()
            torch.cuda.synchronize()
            sec = timed(r, lambda: capi._check(L.cap_winding_numbers(r.ctx, pts.data_ptr(), n, a.beta, w.data_ptr(), visits.data_ptr()), "cap_winding_numbers"),
                        a.reps, a.warmup)
            mean = visits.double().mean(0).cpu().numpy()
            if a.instances is not None:
                inside_flat = w >= 0.5
                isec = timed(r, lambda: capi._check(L.cap_winding_instances(r.ctx, pts.data_ptr(), n, a.beta, w.data_ptr(), visits4.data_ptr()),
                                                    "cap_winding_instances"), a.reps, a.warmup)
                mean4 = visits4.double().mean(0).cpu().numpy()
                print(json.dumps(dict(head, set=name, beta=a.beta, instances=a.instances, contributing=int(wi.contributing), tlas_depth=int(info_i.tlas_depth),
                                      ms=round(isec * 1e3, 3), mpoints_per_s=round(n / isec / 1e6, 2), mean_visits=[round(float(x), 2) for x in mean4],
                                      inside=round(float((w >= 0.5).float().mean()), 4), derived_build_ms=round(derived_ms, 3), flat_ms=round(sec * 1e3, 3),
                                      flat_mpoints_per_s=round(n / sec / 1e6, 2), flat_mean_visits=[round(float(mean[0]), 2), round(float(mean[1]), 2)],
                                      flat_inside=round(float(inside_flat.float().mean()), 4), ratio_to_flat=round(sec / isec, 3),
                                      table_build_ms=round(wn.ms, 3))), flush=True)
                continue
            print(json.dumps(dict(head, set=name, beta=a.beta, ms=round(sec * 1e3, 3), mpoints_per_s=round(n / sec / 1e6, 2),
                                  mean_visits=[round(float(mean[0]), 2), round(float(mean[1]), 2)], inside=round(float((w >= 0.5).float().mean()), 4),
                                  table_build_ms=round(wn.ms, 3), bvh_build_ms=round(info.build_ms, 3),
                                  table={k: v for k, v in wn.as_dict().items() if k != "ms"})), flush=True)
        r.close()
        return
    if a.sweeps:
        # one sweep per point towards a fixed pseudo-random direction (unit length, tmax inf), and cap_trace_rays on the same origins and
        # directions from the same process as the yardstick
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        hits4 = torch.empty((n, 4), dtype=torch.float32, device=dev)
        for name, xyz in sets:
            sw = torch.as_tensor(capi.Renderer.sweep_queries(xyz, a.radius, d), device=dev).contiguous()
            ry = sw.clone()
            ry[:, 3] = 0.0  # (the radius word is a ray's tmin)
            torch.cuda.synchronize()
            sec = timed(r, lambda: capi._check(L.cap_sweep_spheres(r.ctx, sw.data_ptr(), n, out.data_ptr(), None), "cap_sweep_spheres"), a.reps, a.warmup)
            rsec = timed(r, lambda: capi._check(L.cap_trace_rays(r.ctx, ry.data_ptr(), n, hits4.data_ptr(), 0), "cap_trace_rays"), a.reps, a.warmup)
            ids = out[:n, 6].contiguous().view(torch.int32)
            miss = ids == -1
            start = (~miss) & (out[:n, 3] == 0)
            line = dict(head, set=name, radius_frac=a.radius / size, ms=round(sec * 1e3, 3), msweeps_per_s=round(n / sec / 1e6, 2),
                        misses=round(float(miss.float().mean()), 4), start_overlaps=round(float(start.float().mean()), 4),
                        rays_ms=round(rsec * 1e3, 3), mrays_per_s=round(n / rsec / 1e6, 2),
                        ray_misses=round(float((hits4[:, 3].contiguous().view(torch.int32) == -1).float().mean()), 4), ratio_to_rays=round(rsec / sec, 3))
            if a.instances is not None:
                # cap_sweep_instances on the same world sweeps (the point sets lie in instance 0, the identity) under the --instances layout;
                # from the same process the scene form above, the instanced walk over ONE identity instance -- what the two-level loop
                # and the per-node world boxes cost by themselves -- and cap_closest_instances on the origins
                call = lambda: capi._check(L.cap_sweep_instances(r.ctx, sw.data_ptr(), n, flat_out.data_ptr(), inst.data_ptr(), None), "cap_sweep_instances")
                r.set_instances(M[:1])
                one_sec = timed(r, call, a.reps, a.warmup)
                same = bool((flat_out[:n].view(torch.int32) == out[:n].view(torch.int32)).all())
                r.set_instances(M)
                isec = timed(r, call, a.reps, a.warmup)
                imiss = inst[:n] == -1
                istart = (~imiss) & (flat_out[:n, 3] == 0)
                in_identity = float((inst[:n] == 0).float().mean())
                pts = sw[:, 0:4].clone().contiguous()
                pts[:, 3] = float("inf")
                torch.cuda.synchronize()
                csec = timed(r, lambda: capi._check(L.cap_closest_instances(r.ctx, pts.data_ptr(), n, flat_out.data_ptr(), inst.data_ptr(), None),
                                                    "cap_closest_instances"), a.reps, a.warmup)
                line = dict(head, set=name, radius_frac=a.radius / size, instances=a.instances, inert=int(info_i.inert), tlas_depth=int(info_i.tlas_depth),
                            ms=round(isec * 1e3, 3), msweeps_per_s=round(n / isec / 1e6, 2), misses=round(float(imiss.float().mean()), 4),
                            start_overlaps=round(float(istart.float().mean()), 4), in_identity=round(in_identity, 4),
                            identity_ms=round(one_sec * 1e3, 3), identity_msweeps_per_s=round(n / one_sec / 1e6, 2), identity_same_as_scene=same,
                            scene_ms=line["ms"], scene_msweeps_per_s=line["msweeps_per_s"], identity_to_scene=round(sec / one_sec, 3),
                            ratio_to_scene=round(sec / isec, 3), closest_ms=round(csec * 1e3, 3), closest_mpoints_per_s=round(n / csec / 1e6, 2),
                            ratio_to_closest=round(csec / isec, 3))
            print(json.dumps(line), flush=True)
        r.close()
        return
    if a.triangles:
        k = a.k
        if k == 0 and not a.counts:
            ap.error("--triangles --k 0 needs --counts")
        ids = torch.empty((n * max(k, 1),), dtype=torch.int32, device=dev)
        tri_cnt, box_cnt = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        head.update(k=k, counts=a.counts, extent=a.extent)
        del head["radius"]
        for name, xyz in sets:
            v = (xyz[:, None, :] + (rng.random((n, 3, 3)) - 0.5) * a.extent * size).astype(np.float32)
            qs = torch.as_tensor(capi.Renderer.triangle_queries(v[:, 0], v[:, 1], v[:, 2]), device=dev).contiguous()
            b = np.zeros((n, 8), np.float32)
            b[:, 0:3], b[:, 4:7] = v.min(1), v.max(1)
            boxes = torch.as_tensor(b, device=dev).contiguous()
            torch.cuda.synchronize()
            sec = timed(r, lambda: capi._check(L.cap_overlap_triangles(r.ctx, qs.data_ptr(), n, k, ids.data_ptr() if k else None,
                                                                       tri_cnt.data_ptr() if a.counts else None, 0, None), "cap_overlap_triangles"), a.reps, a.warmup)
            bsec = timed(r, lambda: capi._check(L.cap_overlap_boxes(r.ctx, boxes.data_ptr(), n, k, ids.data_ptr() if k else None,
                                                                    box_cnt.data_ptr() if a.counts else None, 0, None), "cap_overlap_boxes"), a.reps, a.warmup)
            capi._check(L.cap_overlap_triangles(r.ctx, qs.data_ptr(), n, 0, None, tri_cnt.data_ptr(), 0, None), "cap_overlap_triangles")
            if a.instances is not None:
                # cap_overlap_triangles_instances on the same world triangles (the point sets lie in instance 0, the identity), beside the flat
                # rate above and cap_overlap_instances on the triangles' bounding boxes
                r.sync()
                flat_mean = float(tri_cnt.double().mean())
                isec = timed(r, lambda: capi._check(L.cap_overlap_triangles_instances(r.ctx, qs.data_ptr(), n, k, ids.data_ptr() if k else None,
                                                                                      inst.data_ptr() if k else None, tri_cnt.data_ptr() if a.counts else None,
                                                                                      0, None), "cap_overlap_triangles_instances"), a.reps, a.warmup)
                bsec = timed(r, lambda: capi._check(L.cap_overlap_instances(r.ctx, boxes.data_ptr(), n, k, ids.data_ptr() if k else None,
                                                                            inst.data_ptr() if k else None, box_cnt.data_ptr() if a.counts else None, 0, None),
                                                    "cap_overlap_instances"), a.reps, a.warmup)
                capi._check(L.cap_overlap_triangles_instances(r.ctx, qs.data_ptr(), n, 0, None, None, tri_cnt.data_ptr(), 0, None),
                            "cap_overlap_triangles_instances")
                capi._check(L.cap_overlap_instances(r.ctx, boxes.data_ptr(), n, 0, None, None, box_cnt.data_ptr(), 0, None), "cap_overlap_instances")
                r.sync()
                print(json.dumps(dict(head, set=name, instances=a.instances, inert=int(info_i.inert), tlas_depth=int(info_i.tlas_depth), ms=round(isec * 1e3, 3),
                                      mtriangles_per_s=round(n / isec / 1e6, 2), mean_pairs=round(float(tri_cnt.double().mean()), 3),
                                      empty=round(float((tri_cnt == 0).float().mean()), 4), flat_ms=round(sec * 1e3, 3),
                                      flat_mtriangles_per_s=round(n / sec / 1e6, 2), flat_mean_candidates=round(flat_mean, 3), ratio_to_flat=round(sec / isec, 3),
                                      boxes_ms=round(bsec * 1e3, 3), mboxes_per_s=round(n / bsec / 1e6, 2),
                                      boxes_mean_pairs=round(float(box_cnt.double().mean()), 3), ratio_to_boxes=round(bsec / isec, 3))), flush=True)
                continue
            capi._check(L.cap_overlap_boxes(r.ctx, boxes.data_ptr(), n, 0, None, box_cnt.data_ptr(), 0, None), "cap_overlap_boxes")
            r.sync()
            print(json.dumps(dict(head, set=name, ms=round(sec * 1e3, 3), mtriangles_per_s=round(n / sec / 1e6, 2),
                                  mean_candidates=round(float(tri_cnt.double().mean()), 3), empty=round(float((tri_cnt == 0).float().mean()), 4),
                                  boxes_ms=round(bsec * 1e3, 3), mboxes_per_s=round(n / bsec / 1e6, 2),
                                  boxes_mean_candidates=round(float(box_cnt.double().mean()), 3), ratio_to_boxes=round(bsec / sec, 3))), flush=True)
        r.close()
        return
    if a.boxes:
        k = a.k
        if k == 0 and not a.counts:
            ap.error("--boxes --k 0 needs --counts")
        half = a.extent * size
        ids = torch.empty((n * max(k, 1),), dtype=torch.int32, device=dev)
        box_cnt, near_cnt = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        head.update(k=k, counts=a.counts, extent=a.extent)
        del head["radius"]
        for name, xyz in sets:
            b = np.zeros((n, 8), np.float32)
            b[:, 0:3], b[:, 4:7] = xyz - half, xyz + half
            boxes = torch.as_tensor(b, device=dev).contiguous()
            q = np.zeros((n, 4), np.float32)
            q[:, 0:3] = xyz
            torch.cuda.synchronize()
            sec = timed(r, lambda: capi._check(L.cap_overlap_boxes(r.ctx, boxes.data_ptr(), n, k, ids.data_ptr() if k else None,
                                                                   box_cnt.data_ptr() if a.counts else None, 0, None), "cap_overlap_boxes"), a.reps, a.warmup)
            capi._check(L.cap_overlap_boxes(r.ctx, boxes.data_ptr(), n, 0, None, box_cnt.data_ptr(), 0, None), "cap_overlap_boxes")
            r.sync()
            mean = float(box_cnt.double().mean())
            if a.instances is not None:
                # cap_overlap_instances on the same world boxes (the point sets lie in instance 0, the identity), beside the flat rate above
                isec = timed(r, lambda: capi._check(L.cap_overlap_instances(r.ctx, boxes.data_ptr(), n, k, ids.data_ptr() if k else None,
                                                                            inst.data_ptr() if k else None, box_cnt.data_ptr() if a.counts else None, 0, None),
                                                    "cap_overlap_instances"), a.reps, a.warmup)
                capi._check(L.cap_overlap_instances(r.ctx, boxes.data_ptr(), n, 0, None, None, box_cnt.data_ptr(), 0, None), "cap_overlap_instances")
                r.sync()
                print(json.dumps(dict(head, set=name, instances=a.instances, inert=int(info_i.inert), tlas_depth=int(info_i.tlas_depth), ms=round(isec * 1e3, 3),
                                      mboxes_per_s=round(n / isec / 1e6, 2), mean_candidates=round(float(box_cnt.double().mean()), 3),
                                      empty=round(float((box_cnt == 0).float().mean()), 4), flat_ms=round(sec * 1e3, 3),
                                      flat_mboxes_per_s=round(n / sec / 1e6, 2), flat_mean_candidates=round(mean, 3), ratio_to_flat=round(sec / isec, 3))), flush=True)
                continue
            # the nearest existing workload: cap_closest_points_multi --counts at the radius with the same mean candidate count (bisection)
            rlo, rhi = 0.0, 4.0 * half
            for _ in range(16):
                q[:, 3] = 0.5 * (rlo + rhi)
                pts = torch.as_tensor(q, device=dev).contiguous()
                torch.cuda.synchronize()
                capi._check(L.cap_closest_points_multi(r.ctx, pts.data_ptr(), n, 0, None, near_cnt.data_ptr(), 0, None), "cap_closest_points_multi")
                r.sync()
                if float(near_cnt.double().mean()) < mean:
                    rlo = 0.5 * (rlo + rhi)
                else:
                    rhi = 0.5 * (rlo + rhi)
            near_mean = float(near_cnt.double().mean())
            near_sec = timed(r, lambda: capi._check(L.cap_closest_points_multi(r.ctx, pts.data_ptr(), n, k, out.data_ptr() if k else None, near_cnt.data_ptr(), 0, None),
                                                    "cap_closest_points_multi"), a.reps, a.warmup)
            print(json.dumps(dict(head, set=name, ms=round(sec * 1e3, 3), mboxes_per_s=round(n / sec / 1e6, 2), mean_candidates=round(mean, 3),
                                  empty=round(float((box_cnt == 0).float().mean()), 4), closest_multi_counts_radius=float(q[0, 3]),
                                  closest_multi_counts_mean_candidates=round(near_mean, 3), closest_multi_counts_ms=round(near_sec * 1e3, 3),
                                  closest_multi_counts_mpoints_per_s=round(n / near_sec / 1e6, 2), ratio_to_closest_multi_counts=round(near_sec / sec, 3))), flush=True)
        r.close()
        return
    if a.k is not None:
        head.update(k=a.k, counts=a.counts)
    for name, xyz in sets:
        q = np.zeros((n, 4), np.float32)
        q[:, 0:3], q[:, 3] = xyz, a.radius
        pts = torch.as_tensor(q, device=dev).contiguous()
        torch.cuda.synchronize()
        if inst_signed:
            flat = lambda: capi._check(L.cap_closest_points(r.ctx, pts.data_ptr(), n, flat_out.data_ptr(), None), "cap_closest_points")
            flat_sec = timed(r, flat, a.reps, a.warmup)
            single = lambda: capi._check(L.cap_closest_instances(r.ctx, pts.data_ptr(), n, flat_out.data_ptr(), plain_inst.data_ptr(), None), "cap_closest_instances")
            single_sec = timed(r, single, a.reps, a.warmup)
            call = lambda: capi._check(L.cap_signed_distance_instances(r.ctx, pts.data_ptr(), n, out.data_ptr(), inst.data_ptr(), signed.data_ptr(), None),
                                       "cap_signed_distance_instances")
        elif inst_multi:
            flat = lambda: capi._check(L.cap_closest_points_multi(r.ctx, pts.data_ptr(), n, a.k, flat_out.data_ptr() if a.k else None,
                                                                  flat_cnt.data_ptr() if a.counts else None, 0, None), "cap_closest_points_multi")
            flat_sec = timed(r, flat, a.reps, a.warmup)
            single = lambda: capi._check(L.cap_closest_instances(r.ctx, pts.data_ptr(), n, single_out.data_ptr(), None, None), "cap_closest_instances")
            single_sec = timed(r, single, a.reps, a.warmup)
            call = lambda: capi._check(L.cap_closest_instances_multi(r.ctx, pts.data_ptr(), n, a.k, out.data_ptr() if a.k else None,
                                                                     inst.data_ptr() if a.k else None, cnt.data_ptr() if a.counts else None, 0, None),
                                       "cap_closest_instances_multi")
        elif a.instances is not None:
            flat = lambda: capi._check(L.cap_closest_points(r.ctx, pts.data_ptr(), n, flat_out.data_ptr(), None), "cap_closest_points")
            flat_sec = timed(r, flat, a.reps, a.warmup)
            call = lambda: capi._check(L.cap_closest_instances(r.ctx, pts.data_ptr(), n, out.data_ptr(), inst.data_ptr(), None), "cap_closest_instances")
        elif a.signed:
            flat = lambda: capi._check(L.cap_closest_points(r.ctx, pts.data_ptr(), n, flat_out.data_ptr(), None), "cap_closest_points")
            flat_sec = timed(r, flat, a.reps, a.warmup)
            call = lambda: capi._check(L.cap_signed_distance(r.ctx, pts.data_ptr(), n, out.data_ptr(), signed.data_ptr(), None), "cap_signed_distance")
        elif a.k is None:
            call = lambda: capi._check(L.cap_closest_points(r.ctx, pts.data_ptr(), n, out.data_ptr(), None), "cap_closest_points")
        else:
            call = lambda: capi._check(L.cap_closest_points_multi(r.ctx, pts.data_ptr(), n, a.k, out.data_ptr() if a.k else None,
                                                                  cnt.data_ptr() if a.counts else None, 0, None), "cap_closest_points_multi")
        sec = timed(r, call, a.reps, a.warmup)
        line = dict(head, set=name, ms=round(sec * 1e3, 3), mpoints_per_s=round(n / sec / 1e6, 1))
        if a.k != 0:
            page = out.cpu().numpy().reshape(n, -1, 8)
            listed = page.view(np.uint32)[:, :, 6] != capi.MISS
            rec, hit = page[:, 0], listed[:, 0]
            line.update(hits=round(float(hit.mean()), 4),
                        mean_dist=round(float(np.sqrt(rec[hit, 3].astype(np.float64)).mean() / size), 5) if hit.any() else None)
        if inst_signed:
            same = (out.view(torch.int32) == flat_out.view(torch.int32)).all(1) & (inst == plain_inst)
            sd = signed.cpu().numpy()
            line.update(instances=a.instances, inert=int(info_i.inert), tlas_depth=int(info_i.tlas_depth), unsigned_ms=round(single_sec * 1e3, 3),
                        unsigned_mpoints_per_s=round(n / single_sec / 1e6, 1), time_over_unsigned=round(sec / single_sec, 4), flat_ms=round(flat_sec * 1e3, 3),
                        extra_over_flat=round((sec - single_sec) / flat_sec, 4), same_records=round(float(same.float().mean()), 4),
                        in_identity=round(float((inst == 0).float().mean()), 4), negative=round(float((sd[hit] < 0).mean()), 4) if hit.any() else None,
                        table_build_ms=round(pn.ms, 3))
        elif inst_multi:
            line.update(instances=a.instances, inert=int(info_i.inert), tlas_depth=int(info_i.tlas_depth), flat_ms=round(flat_sec * 1e3, 3),
                        flat_mpoints_per_s=round(n / flat_sec / 1e6, 1), ratio_to_flat=round(flat_sec / sec, 3), single_ms=round(single_sec * 1e3, 3),
                        single_mpoints_per_s=round(n / single_sec / 1e6, 1), ratio_to_single=round(single_sec / sec, 3))
            if a.k:
                alone = (inst.view(n, a.k) <= 0).all(1)  # the identity instance or a miss in every slot: no neighbour reaches the page
                equal = (out.view(torch.int32).view(n, -1) == flat_out.view(torch.int32).view(n, -1)).all(1)
                line.update(flat_comparable=round(float(alone.float().mean()), 4),
                            same_as_flat=round(float(equal[alone].float().mean()), 4) if bool(alone.any()) else None)
        elif a.instances is not None:
            same = float((out.view(torch.int32) == flat_out.view(torch.int32)).all(1).float().mean())
            line.update(instances=a.instances, inert=int(info_i.inert), tlas_depth=int(info_i.tlas_depth), flat_ms=round(flat_sec * 1e3, 3),
                        flat_mpoints_per_s=round(n / flat_sec / 1e6, 1), ratio_to_flat=round(flat_sec / sec, 3), same_as_flat=round(same, 4))
        if a.signed and not inst_signed:
            same = float((out.view(torch.int32) == flat_out.view(torch.int32)).all(1).float().mean())
            sd = signed.cpu().numpy()
            line.update(flat_ms=round(flat_sec * 1e3, 3), flat_mpoints_per_s=round(n / flat_sec / 1e6, 1), time_over_flat=round(sec / flat_sec, 4),
                        same_records=round(same, 4), negative=round(float((sd[hit] < 0).mean()), 4) if hit.any() else None,
                        table_build_ms=round(pn.ms, 3), bvh_build_ms=round(info.build_ms, 3), weld={k: v for k, v in pn.as_dict().items() if k != "ms"})
        if a.k is not None:
            line.update(mean_candidates=round(float(cnt.cpu().numpy().astype(np.float64).mean() if a.counts else listed.sum(1).mean()), 3))
        print(json.dumps(line), flush=True)
    if a.instances is not None or a.signed:
        r.close()
        return
    rays = torch.as_tensor(random_rays(lo, hi, n, rng), device=dev).contiguous()
    hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sec = timed(r, lambda: capi._check(L.cap_trace_rays(r.ctx, rays.data_ptr(), n, hits.data_ptr(), 0), "cap_trace_rays"), a.reps, a.warmup)
    print(json.dumps(dict(head, set="random rays (cap_trace_rays)", ms=round(sec * 1e3, 3), mrays_per_s=round(n / sec / 1e6, 1))), flush=True)
    r.close()


if __name__ == "__main__":
    main()
