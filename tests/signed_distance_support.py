"""Helpers of the signed-distance tests (cap_pseudonormals_build, cap_signed_distance): a float64 reference of the pseudonormal table of
include/capsaicin_hip.h ("signed distance") -- the weld by np.unique on the coordinate bits, the sums by plain loops in (triangle,
corner) order --, the float32 sign computation of the query on closest_point_support.closest, the float64 winding number (Van
Oosterom & Strackee's solid angle summed over the triangles) as ground truth, and the test meshes, all wound outwards."""
import functools

import numpy as np

from closest_point_support import around, bits, closest, records_of, sphere

MISS = 0xFFFFFFFF
STATS = ("vertices", "edges", "boundary_edges", "nonmanifold_edges", "inconsistent_edges", "degenerate_triangles", "closed")


# ---- the table, float64 ----
def _angle(a, b):
    c = np.cross(a, b)
    return np.arctan2(np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])


def pseudonormals(tris):
    """(table (T, 7, 3) float64, statistics) of (T, 3, 3) float32 triangles in global id order"""
    with np.errstate(invalid="ignore"):
        p32 = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3) + np.float32(0.0)  # -0 -> +0
    T = len(p32)
    P = p32.astype(np.float64)
    finite = np.isfinite(P).all((1, 2))
    with np.errstate(all="ignore"):
        n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    live = finite & (n != 0).any(1)
    # weld ids of the corners: equal coordinate bits (two corners of one triangle at one position leave no cross product: not live)
    _, weld = np.unique(p32.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    weld = weld.reshape(T, 3)
    for g in np.nonzero(live)[0]:
        assert len(set(weld[g])) == 3
    table = np.zeros((T, 7, 3), np.float64)
    vsum, esum, members = {}, {}, {}
    for g in np.nonzero(live)[0]:
        nf = n[g] / np.sqrt((n[g, 0] * n[g, 0] + n[g, 1] * n[g, 1]) + n[g, 2] * n[g, 2])
        table[g, 0] = nf
        for k in range(3):
            a, b = P[g, (k + 1) % 3] - P[g, k], P[g, (k + 2) % 3] - P[g, k]
            w = weld[g, k]
            vsum[w] = vsum.get(w, np.zeros(3)) + _angle(a, b) * nf
            w1 = weld[g, (k + 1) % 3]
            e = (min(w, w1), max(w, w1))
            esum[e] = esum.get(e, np.zeros(3)) + nf
            members.setdefault(e, []).append(w < w1)
    for g in np.nonzero(live)[0]:
        for k in range(3):
            w, w1 = weld[g, k], weld[g, (k + 1) % 3]
            table[g, 1 + k] = esum[(min(w, w1), max(w, w1))]
            table[g, 4 + k] = vsum[w]
    s = dict(vertices=len(vsum), edges=len(esum), boundary_edges=sum(len(m) == 1 for m in members.values()),
             nonmanifold_edges=sum(len(m) > 2 for m in members.values()),
             inconsistent_edges=sum(len(m) == 2 and bool(m[0] == m[1]) for m in members.values()), degenerate_triangles=int(T - live.sum()))
    s["closed"] = int(s["boundary_edges"] == 0 and s["nonmanifold_edges"] == 0 and s["inconsistent_edges"] == 0 and live.any())
    return table, s


def assert_table(dev, ref, what=""):
    """per entry |dev - ref|_inf <= 2^-23 |ref|_inf -- one binary32 rounding is 2^-24 of the largest component, the factor 2 covers a
    differing atan2 ulp, the float64 sums are negligible -- and an entry that is zero in the reference is exactly zero"""
    dev = np.asarray(dev, np.float64).reshape(-1, 3)
    ref = np.asarray(ref, np.float64).reshape(-1, 3)
    assert dev.shape == ref.shape, what
    err, mag = np.abs(dev - ref).max(1), np.abs(ref).max(1)
    bad = np.nonzero(~(err <= 2.0 ** -23 * mag))[0]
    assert len(bad) == 0, "%s: %d of %d entries off, first %d (triangle %d, entry %d): %s against %s" % (
        what, len(bad), len(ref), bad[0], bad[0] // 7, bad[0] % 7, dev[bad[0]].tolist(), ref[bad[0]].tolist())


def stats_of(info):
    return {k: int(getattr(info, k)) for k in STATS}


# ---- the query's sign, float32 ----
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def signed_of(records, points, tris, table32):
    """cap_signed_distance's float32 array for (N, 8) records of closest_point_support.closest: delta recomputed from the record's
    (u, v), dotted with the float32 table entry of (triangle, feature)"""
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, 8)
    q = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    table32 = np.ascontiguousarray(table32, np.float32).reshape(-1, 7, 3)
    v0, e1, e2 = records_of(np.ascontiguousarray(tris, np.float32))
    g, f = bits(rec)[:, 6].astype(np.int64), bits(rec)[:, 7].astype(np.int64)
    hit = g != MISS
    out = np.full(len(rec), np.inf, np.float32)
    gh, u, v = g[hit], rec[hit, 4:5], rec[hit, 5:6]
    ap = q[hit, 0:3] - v0[gh]
    delta = ap - (e1[gh] * u + e2[gh] * v)
    d = _dot(delta, table32[gh, f[hit]])
    dist = np.sqrt(rec[hit, 3])
    assert delta.dtype == np.float32 and d.dtype == np.float32 and dist.dtype == np.float32
    out[hit] = np.where(d < 0, -dist, dist)
    return out


def signed_distance(points, tris, table32, mask=None):
    """(records, signed) expected of cap_signed_distance"""
    rec, _ = closest(points, tris, mask)
    return rec, signed_of(rec, points, tris, table32)


def face_normal_sign(records, points, tris):
    """the shortcut the table replaces: the sign of dot(p - q, face normal of the returned triangle), in float64; +1 / -1"""
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, 8)
    g = bits(rec)[:, 6].astype(np.int64)
    t = np.asarray(tris, np.float64)[g]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    d = ((np.asarray(points, np.float64)[:, 0:3] - rec[:, 0:3].astype(np.float64)) * n).sum(1)
    return np.where(d < 0, -1, 1)


# ---- ground truth ----
def winding_number(points, tris, chunk=512):
    """the float64 winding number of (N, 3) points about (T, 3, 3) triangles: 1 inside a closed mesh wound outwards, 0 outside"""
    p = np.asarray(points, np.float64)[:, 0:3]
    t = np.asarray(tris, np.float64)
    out = np.zeros(len(p))
    for s in range(0, len(p), chunk):
        q = p[s:s + chunk, None, None, :]
        a, b, c = (t[None, :, k] - q[:, :, 0] for k in range(3))
        la, lb, lc = (np.linalg.norm(x, axis=2) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(2)
        den = la * lb * lc + (a * b).sum(2) * lc + (b * c).sum(2) * la + (c * a).sum(2) * lb
        out[s:s + chunk] = (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)
    return out


# ---- meshes, wound outwards ----
def outward(tris):
    """the triangles of a convex mesh, each turned to face away from the mesh's centre"""
    t = np.array(tris, np.float64)
    centre = t.reshape(-1, 3).mean(0)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    flip = (n * (t.mean(1) - centre)).sum(1) < 0
    t[flip] = t[flip][:, [0, 2, 1]]
    return t.astype(np.float32)


def tetrahedron():
    v = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float64)
    return outward([v[[0, 1, 2]], v[[0, 1, 3]], v[[0, 2, 3]], v[[1, 2, 3]]])


def octahedron():
    return outward([[(sx, 0, 0), (0, sy, 0), (0, 0, sz)] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])


def box(size=(1.0, 2.0, 3.0), split=0, origin=(0.0, 0.0, 0.0)):
    """12 triangles; bit k of `split` picks the diagonal of face k"""
    out = []
    face = 0
    for axis in range(3):
        for side in (0, 1):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            c = np.zeros((4, 3))
            c[:, axis] = side * size[axis]
            c[:, u] = np.array([0, 1, 1, 0]) * size[u]
            c[:, v] = np.array([0, 0, 1, 1]) * size[v]
            c += np.array(origin)
            out += [c[[0, 1, 2]], c[[0, 2, 3]]] if not (split >> face) & 1 else [c[[0, 1, 3]], c[[1, 2, 3]]]
            face += 1
    return outward(out)


def torus(major=16, minor=8, R=1.0, r=0.4):
    def at(i, j):
        a, b = 2 * np.pi * (i % major) / major, 2 * np.pi * (j % minor) / minor
        return np.array([(R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)])
    out = []
    for i in range(major):
        for j in range(minor):
            p00, p10, p11, p01 = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            out += [(p00, p10, p11), (p00, p11, p01)]
    return np.array(out).astype(np.float32)


def cone(valence=300):
    """a closed cone: an apex and a base centre of the given valence (a run longer than a wave and than a workgroup)"""
    a = 2 * np.pi * np.arange(valence + 1) / valence
    ring = np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], 1)
    ring[valence] = ring[0]
    apex, centre = np.array([0.0, 0.0, 1.0]), np.zeros(3)
    out = [(apex, ring[i], ring[i + 1]) for i in range(valence)] + [(centre, ring[i + 1], ring[i]) for i in range(valence)]
    return np.array(out).astype(np.float32)


MESHES = {
    "tetrahedron": tetrahedron,
    "octahedron": octahedron,
    "box": box,
    "torus": torus,
    "sphere": lambda: sphere(12, 12),
    "cone": cone,
    "sphere soup": lambda: sphere(50, 50),  # 14 700 corners: several 2 048-element sort tiles
}
TRUTH_MESHES = tuple(MESHES)[:6]


@functools.lru_cache(maxsize=None)
def mesh(name):
    t = MESHES[name]()
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def reference_table(name):
    table, stats = pseudonormals(mesh(name))
    table.setflags(write=False)
    return table, stats


@functools.lru_cache(maxsize=None)
def truth_case(name):
    """4 000 points around the mesh (seed 7), those at least 10^-3 of the box diagonal from it kept: (queries, records, inside, kept
    indices).  The distance bound is a choice of inputs; no kept point is excused."""
    tris = mesh(name)
    rng = np.random.default_rng(7)
    q = np.zeros((4000, 4), np.float32)
    q[:, 0:3], q[:, 3] = around(rng, tris, 4000, 0.5), np.inf
    rec, _ = closest(q, tris)
    v = tris.reshape(-1, 3).astype(np.float64)
    diag = np.linalg.norm(v.max(0) - v.min(0))
    keep = np.nonzero(np.sqrt(rec[:, 3].astype(np.float64)) >= 1e-3 * diag)[0]
    w = winding_number(q[keep], tris)
    assert (np.abs(w - np.round(w)) < 1e-6).all() and set(np.round(w).astype(int)) <= {0, 1}
    inside = np.round(w).astype(int) == 1
    for a in (q, rec):
        a.setflags(write=False)
    return q, rec, inside, keep


# ---- uploads ----
def indexed_arrays(*meshes):
    """GeometryStorage arrays of one mesh per (vertices (V, 3), faces (F, 3)) pair"""
    P, I, D = [], [], []
    fv = fi = 0
    for verts, faces in meshes:
        verts, faces = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.uint32).reshape(-1)
        P.append(verts)
        I.append(faces)
        D.append([len(verts), fv, len(faces), fi, len(D), 0xFFFFFFFF, 0, 0])
        fv += len(verts)
        fi += len(faces)
    P = np.concatenate(P)
    N = np.tile(np.float32([0, 0, 1]), (len(P), 1))
    return P, N, np.zeros((len(P), 2), np.float32), np.concatenate(I), np.array(D, np.uint32)


def indexed(tris):
    """(vertices, faces) of a triangle list with equal positions shared"""
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3)
    _, first, inverse = np.unique(t.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    return t[first], inverse.reshape(-1, 3).astype(np.uint32)
