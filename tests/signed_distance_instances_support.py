"""Helpers of the instanced signed-distance tests (cap_signed_distance_instances): the float32 reference of include/capsaicin_hip.h
("signed distance over instances") -- closest_instances_support.closest_instances for the world record, p' = W p in single-rounded
float32 operations from a GIVEN W, closest_point_support.closest restricted to the winning instance's candidates for the sign record,
signed_distance_support.signed_of on a GIVEN float32 table, and the rule for the signed value --, a scene of closed objects placed apart
with its object ranges, and the float64 winding number about the winning instance's transformed mesh as ground truth."""
import functools

import numpy as np

from closest_instances_support import MISS, assert_pairs, bits, bound, closest_instances, pair_valid  # noqa: F401
from closest_point_support import arrays, closest, queries
from instance_support import regular_transforms
from signed_distance_support import cone, pseudonormals, signed_of, tetrahedron, torus, winding_number


# ---- the reference, float32 ----
def to_object(W, xyz):
    """p' of the contract for (N, 3) float32 points under one stored W (3, 4): per row ((W_r0 x + W_r1 y) + W_r2 z) + W_r3, every
    operation one rounded float32 operation"""
    W = np.asarray(W, np.float32).reshape(3, 4)
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        out = np.stack([((W[r, 0] * p[:, 0] + W[r, 1] * p[:, 1]) + W[r, 2] * p[:, 2]) + W[r, 3] for r in range(3)], 1)
    assert out.dtype == np.float32
    return out


def stored_inverse(M):
    """the W cap_instances_set stores for the (I, 3, 4) transforms, through the library's host routine (the debug entry)"""
    return np.stack([bound(m, (0, 0, 0), (0, 0, 0), (0, 0, 0), 0.0)["W"] for m in np.asarray(M, np.float32).reshape(-1, 3, 4)])


def signed_distance_instances(points, M, W, tris, table32, valid=None, world=None, sign_valid=None):
    """(records (N, 8) float32, instances (N,) int32 with -1 on a miss, signed (N,) float32) expected of
    cap_signed_distance_instances.  W: the stored world-to-object matrices (I, 3, 4), table32: the float32 pseudonormal table, valid:
    (I, T) bool from pair_valid (None = every pair).  world: closest_instances(points, M, tris, valid) where the caller has it already
    (it depends on neither W nor the table).  sign_valid: other candidates for the sign walk than the contract's, to show what a walk
    that ignored them would answer."""
    q = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    tris = np.ascontiguousarray(tris, np.float32)
    M = np.asarray(M, np.float32).reshape(-1, 3, 4)
    W = np.asarray(W, np.float32).reshape(-1, 3, 4)
    if valid is None:
        valid = np.ones((len(M), len(tris)), bool)
    rec, inst = closest_instances(q, M, tris, valid) if world is None else world
    if sign_valid is None:
        sign_valid = valid
    negative = np.zeros(len(q), bool)
    for i in np.unique(inst[inst >= 0]):
        idx = np.nonzero(inst == i)[0]
        # the flat signed query at (p', +inf) over instance i's candidates; an overflowed p' is a degenerate point there: +inf, positive
        qo = queries(to_object(W[i], q[idx, 0:3]))
        sign_rec, _ = closest(qo, tris, sign_valid[i])
        negative[idx] = signed_of(sign_rec, qo, tris, table32) < 0
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(rec[:, 3])
    assert dist.dtype == np.float32
    signed = np.where(negative & (rec[:, 3] != 0), -dist, dist).astype(np.float32)
    signed[inst < 0] = np.inf
    return rec, inst, signed


def assert_signed(got, want, what=""):
    """records bit for bit on all eight words, the instance, and the signed word"""
    assert_pairs(got[:2], want[:2], what)
    g, w = bits(got[2]).reshape(-1), bits(want[2]).reshape(-1)
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, "%s: %d of %d signed distances differ, first %d: got %r want %r" % (
        what, len(bad), len(g), bad[0], float(np.asarray(got[2]).reshape(-1)[bad[0]]), float(np.asarray(want[2]).reshape(-1)[bad[0]]))


# ---- the scene: closed objects placed apart, one mesh each ----
OFFSETS = ((0.0, 0.0, 0.0), (8.0, 0.0, 0.0), (0.0, 8.0, 0.0))


@functools.lru_cache(maxsize=None)
def three_objects():
    """(GeometryStorage arrays, triangles (860, 3, 3), object ranges (3, 2), object of every triangle): a tetrahedron at the origin, a
    torus shifted by (8, 0, 0) and a 300-valent cone shifted by (0, 8, 0).  Apart, because the pseudonormal table welds across the whole
    scene: objects that touch share edges and are no longer closed."""
    parts = [(mesh() + np.float32(off)).astype(np.float32) for mesh, off in zip((tetrahedron, torus, cone), OFFSETS)]
    tris = np.concatenate(parts)
    ranges = np.array([(k, 1) for k in range(len(parts))], np.uint32)
    obj_of_tri = np.concatenate([np.full(len(p), k) for k, p in enumerate(parts)])
    for a in (tris, obj_of_tri):
        a.setflags(write=False)
    return arrays(*parts), tris, ranges, obj_of_tri


@functools.lru_cache(maxsize=None)
def reference_table32():
    """the float32 rounding of the float64 reference table of the three-object scene, and its statistics"""
    table, stats = pseudonormals(three_objects()[1])
    table = table.astype(np.float32)
    table.setflags(write=False)
    return table, stats


def object_box_points(rng, M, tris, obj_of_tri, objects, n, grow=0.1):
    """n world points: point k is the image under instance (k mod I) of a point uniform in its object's box grown by `grow` of its
    extent on every side"""
    Md = np.asarray(M, np.float64)
    t = np.asarray(tris, np.float64)
    i = np.arange(n) % len(Md)
    lo = np.stack([t[obj_of_tri == o].reshape(-1, 3).min(0) for o in objects])[i]
    hi = np.stack([t[obj_of_tri == o].reshape(-1, 3).max(0) for o in objects])[i]
    x = lo - grow * (hi - lo) + rng.random((n, 3)) * (1 + 2 * grow) * (hi - lo)
    return (np.einsum("nrk,nk->nr", Md[i][:, :, :3], x) + Md[i][:, :, 3]).astype(np.float32)


# ---- ground truth ----
def inside_truth(points, inst, M, tris, obj_of_tri=None, objects=None, rel=1e-3, dist2=None):
    """(inside (N,) bool, kept (N,) bool) for the points with a winning instance: |winding number| about that instance's transformed
    mesh in float64 (a mirror negates the number), and whether the point is at least `rel` of the instance's world box diagonal from
    the surface (dist2: the world records' squared distances).  No kept point is excused: the winding number of every one must round
    to 0 or 1 within 1e-6."""
    p = np.asarray(points, np.float64).reshape(-1, 4)[:, 0:3]
    Md = np.asarray(M, np.float64).reshape(-1, 3, 4)
    t = np.asarray(tris, np.float64)
    inside, kept = np.zeros(len(p), bool), np.zeros(len(p), bool)
    for i in np.unique(inst[inst >= 0]):
        idx = np.nonzero(inst == i)[0]
        mine = t if objects is None else t[np.asarray(obj_of_tri) == objects[i]]
        world = np.einsum("rk,tck->tcr", Md[i, :, :3], mine) + Md[i, :, 3]
        diag = np.linalg.norm(world.reshape(-1, 3).max(0) - world.reshape(-1, 3).min(0))
        kept[idx] = np.sqrt(np.asarray(dist2, np.float64)[idx]) >= rel * diag
        k = idx[kept[idx]]
        w = np.abs(winding_number(p[k], world))
        assert (np.abs(w - np.round(w)) < 1e-6).all() and set(np.round(w).astype(int)) <= {0, 1}, "instance %d" % i
        inside[k] = np.round(w).astype(int) == 1
    return inside, kept


@functools.lru_cache(maxsize=None)
def truth_case():
    """The three-object scene under regular_transforms(24), instance k showing object k mod 3, and 1 536 points (seed 11), point k in
    the image of instance (k mod 24)'s grown object box: (queries, M, objects, valid pairs, mirrored (24,) bool)."""
    _, tris, _, obj_of_tri = three_objects()
    M = regular_transforms(24)
    objects = np.arange(24) % 3
    rng = np.random.default_rng(11)
    q = queries(object_box_points(rng, M, tris, obj_of_tri, objects, 1536, 0.1))
    valid = pair_valid(24, len(tris), None, None, None, None, objects, obj_of_tri)
    mirrored = np.linalg.det(M[:, :, :3].astype(np.float64)) < 0
    for a in (q, M, valid):
        a.setflags(write=False)
    return q, M, objects, valid, mirrored


def assert_truth(q, M, objects, mirrored, result, what=""):
    """the signs of (records, instances, signed) against the winding number, under the conditions that keep the test from hiding a
    failure: at least 95 % of the points kept, at least 15 % of the kept ones inside, at least 20 kept inside points in mirrored
    instances"""
    _, tris, _, obj_of_tri = three_objects()
    rec, inst, signed = result
    assert (inst >= 0).all(), what
    inside, kept = inside_truth(q, inst, M, tris, obj_of_tri, objects, 1e-3, rec[:, 3])
    n_kept, n_in, n_mirror = int(kept.sum()), int((kept & inside).sum()), int((kept & inside & mirrored[inst]).sum())
    print("%s: %d of %d points kept, %d inside, %d of those in mirrored instances" % (what, n_kept, len(q), n_in, n_mirror))
    assert n_kept >= 0.95 * len(q) and n_in >= 0.15 * n_kept and n_mirror >= 20, (what, n_kept, n_in, n_mirror)
    wrong = np.nonzero(kept & ((signed < 0) != inside))[0]
    assert len(wrong) == 0, "%s: %d wrong signs, first point %d in instance %d: signed %r, inside %r" % (
        what, len(wrong), wrong[0], inst[wrong[0]], float(signed[wrong[0]]), bool(inside[wrong[0]]))
