"""Helpers of the object tests (cap_objects_set, cap_instances_set_ex): scenes concatenated into one upload with one object per part,
and the brute force of instanced queries over an object table, built on tests/instance_support.py: per object the box-free brute force
of its own triangles under its own instances, merged across objects in (t, instance, triangle) order."""
import numpy as np

from filter_support import mesh_of_triangles
from instance_support import MISS, candidates, closest_record, f32, instanced_hits, instanced_occlusion, merge  # noqa: F401


def concat(parts):
    """[(positions, normals, texcoords, indices, meshes), ...] -> one scene's arrays, parts in order, and the (K, 2) uint32 object
    ranges (first_mesh, mesh_count), one object per part"""
    Ps, Ns, Ts, Is, Ms, ranges = [], [], [], [], [], []
    nv = ni = 0
    for P, N, T, I, M in parts:
        M = np.asarray(M, np.uint32).reshape(-1, 8)
        ranges.append((len(Ms), len(M)))
        for m in M:
            Ms.append([m[0], int(m[1]) + nv, m[2], int(m[3]) + ni, len(Ms), m[5], 0, 0])
        Ps.append(np.asarray(P, f32).reshape(-1, 3)), Ns.append(np.asarray(N, f32).reshape(-1, 3)), Ts.append(np.asarray(T, f32).reshape(-1, 2))
        Is.append(np.asarray(I, np.uint32).ravel())
        nv, ni = nv + len(Ps[-1]), ni + len(Is[-1])
    return (np.concatenate(Ps), np.concatenate(Ns), np.concatenate(Ts), np.concatenate(Is), np.array(Ms, np.uint32)), np.array(ranges, np.uint32)


def triangle_ranges(meshes, ranges):
    """(first_triangle, triangle_count) per object: global triangle ids go mesh by mesh in upload order"""
    per_mesh = np.asarray(meshes, np.uint32).reshape(-1, 8)[:, 2].astype(np.int64) // 3
    begin = np.concatenate([[0], np.cumsum(per_mesh)])
    r = np.asarray(ranges, np.int64).reshape(-1, 2)
    return np.stack([begin[r[:, 0]], begin[r[:, 0] + r[:, 1]] - begin[r[:, 0]]], 1)


def object_candidates(rays, W, live, objects, tris, tri_ranges):
    """per object, instance_support.candidates of its triangles (local ids) under its live instances"""
    objects = np.asarray(objects)
    out = []
    for k, (f, n) in enumerate(tri_ranges):
        lk = live & (objects == k)
        out.append(candidates(rays, W, lk, tris[f:f + n]) if lk.any() else [dict() for _ in range(len(rays))])
    return out


def object_hits(ray, W, live, inst_masks, objects, tris, tri_ranges, mesh_of_tri=None, mesh_masks=None, cull=None, mask=None, cands=None):
    """The filtered hit set of one world ray over the object table in (t, i, g) order as (t, u, v, i, g), g the scene's triangle id.
    objects: (N,) object index per instance; tri_ranges: triangle_ranges(); cands: per object {instance: local triangles} or None."""
    objects = np.asarray(objects)
    per = []
    for k, (f, n) in enumerate(tri_ranges):
        mot = None if mesh_of_tri is None else mesh_of_tri[f:f + n]
        h = instanced_hits(ray, W, live & (objects == k), inst_masks, tris[f:f + n], mot, mesh_masks, cull, mask, None if cands is None else cands[k])
        per += [(i, [(t, u, v, g + int(f))]) for t, u, v, i, g in h]
    return merge(per)


def object_occlusion(ray, W, live, inst_masks, objects, tris, tri_ranges, mesh_of_tri=None, mesh_masks=None, cull=None, mask=None, cands=None):
    objects = np.asarray(objects)
    for k, (f, n) in enumerate(tri_ranges):
        mot = None if mesh_of_tri is None else mesh_of_tri[f:f + n]
        if instanced_occlusion(ray, W, live & (objects == k), inst_masks, tris[f:f + n], mot, mesh_masks, cull, mask, None if cands is None else cands[k]):
            return 1
    return 0


def expected(rays, W, live, inst_masks, objects, tris, tri_ranges, mesh_of_tri=None, mesh_masks=None, cull=None, mask=None, cands=None):
    """(records (N, 4) uint32, instances (N,) uint32, occlusion (N,) int32, hit lists) of the brute force over the object table"""
    if cands is None:
        cands = object_candidates(rays, W, live, objects, tris, tri_ranges)
    rec, inst, occ, lists = [], [], [], []
    for j, ray in enumerate(rays):
        c = [ck[j] for ck in cands]
        h = object_hits(ray, W, live, inst_masks, objects, tris, tri_ranges, mesh_of_tri, mesh_masks, cull, mask, c)
        a, b = closest_record(h, ray[7])
        rec.append(a), inst.append(b), lists.append(h)
        occ.append(object_occlusion(ray, W, live, inst_masks, objects, tris, tri_ranges, mesh_of_tri, mesh_masks, cull, mask, c))
    return np.array(rec, np.uint32).reshape(-1, 4), np.array(inst, np.uint32), np.array(occ, np.int32), lists


def scene_triangles(arrays):
    """(T, 3, 3) float32 vertices in global triangle order of concatenated arrays"""
    P, _, _, I, M = arrays
    out = []
    for d in np.asarray(M, np.uint32).reshape(-1, 8):
        nv, fv, ni, fi = (int(x) for x in d[:4])
        out.append(P[I[fi:fi + (ni // 3) * 3].astype(np.int64) + fv].reshape(-1, 3, 3))
    return np.concatenate(out).astype(f32)


def single_triangle():
    """one mesh of one triangle whose box centre lies inside it: an object without a node"""
    P = np.array([[0, 0, 0], [1, 0, 0.2], [0.5, 1, 0.1]], f32)
    N, T = np.tile(f32([0, 0, 1]), (3, 1)), np.zeros((3, 2), f32)
    return (P, N, T, np.array([0, 1, 2], np.uint32), np.array([[3, 0, 3, 0, 0, 0xFFFFFFFF, 0, 0]], np.uint32))


__all__ = ["MISS", "concat", "triangle_ranges", "object_candidates", "object_hits", "object_occlusion", "expected", "scene_triangles",
           "single_triangle", "mesh_of_triangles"]
