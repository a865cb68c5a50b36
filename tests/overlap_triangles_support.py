"""Helpers of the triangle overlap tests (cap_overlap_triangles): the 17-axis predicate of include/capsaicin_hip.h transcribed to numpy --
one rounded operation per operation of the contract, float32 throughout on the answer path (the same code runs in float64 as the twin) --,
an exact integer intersection test by another method (edge against triangle by signed volumes, a 2-D branch for coplanar edges, Python
ints), the queries that are not traversed, the table of every pair's answer under mask, skip and cursor (overlap_support's Table, pages
and cursors), the lattice scene whose answers float32 gives exactly, and the cases of the GPU tests."""
import functools

import numpy as np

from closest_point_support import around, needles, records_of, soup
from multi_hit_support import stacked_quads
from overlap_support import (MISS, Table, all_miss, assert_counts, assert_pages, boxes_of, cursors_of, fill_classes, ids_of, node_skipped,  # noqa: F401
                             pages, scene_slack)

f32 = np.float32
NONE = 0xFFFFFFFF
AXES = (["n", "m"] + ["f%d x g%d" % (i, j) for j in range(3) for i in range(3)] + ["n x f%d" % i for i in range(3)] + ["m x g%d" % j for j in range(3)])


def queries_of(a, b, c, skip=None):
    """(N, 12) float32 CapTriangleDesc rows of (N, 3) vertices; column 3 holds the bits of skip (NONE by default), the pad words a NaN,
    which nobody may read"""
    a, b, c = (np.asarray(x, f32).reshape(-1, 3) for x in (a, b, c))
    q = np.full((len(a), 12), np.nan, f32)
    q[:, 0:3], q[:, 4:7], q[:, 8:11] = a, b, c
    q.view(np.uint32)[:, 3] = NONE if skip is None else np.asarray(skip, np.int64).astype(np.uint32)
    return q


def queries_of_tris(tris, skip=None):
    t = np.asarray(tris, f32).reshape(-1, 3, 3)
    return queries_of(t[:, 0], t[:, 1], t[:, 2], skip)


def vertices_of(queries):
    """(N, 3, 3) float32 vertices of (N, 12) rows"""
    q = np.ascontiguousarray(queries, f32).reshape(-1, 12)
    return np.stack([q[:, 0:3], q[:, 4:7], q[:, 8:11]], 1)


def skips_of(queries):
    return np.ascontiguousarray(queries, f32).reshape(-1, 12).view(np.uint32)[:, 3].copy()


def _min3(a, b, c):
    return np.minimum(np.minimum(a, b), c)  # (hands a NaN on)


def _max3(a, b, c):
    return np.maximum(np.maximum(a, b), c)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def coordinate_axes(A, v0, e1, e2):
    """step 1 for queries A (N, 3, 3) x records (T, 3): (N, T) bool, True where a coordinate axis separates"""
    with np.errstate(all="ignore"):
        B0, B1, B2 = v0, v0 + e1, v0 + e2
        amin, amax = _min3(A[:, 0], A[:, 1], A[:, 2]), _max3(A[:, 0], A[:, 1], A[:, 2])
        return ((_min3(B0, B1, B2)[None] > amax[:, None]) | (_max3(B0, B1, B2)[None] < amin[:, None])).any(-1)


def axes17(A, v0, e1, e2):
    """steps 2 and 3 pair by pair: A (P, 3, 3) against records (P, 3) each, in the arrays' own dtype: (P, 17) bool in the order of AXES,
    True where that axis separates.  Every axis is evaluated for every pair."""
    dt = A.dtype
    assert v0.dtype == dt and e1.dtype == dt and e2.dtype == dt
    with np.errstate(all="ignore"):
        A0 = A[:, 0]
        B = [v0, v0 + e1, v0 + e2]
        p = [A[:, j] - A0 for j in range(3)]
        q = [B[j] - A0 for j in range(3)]
        f = [p[1], p[2] - p[1], p[0] - p[2]]
        g = [e1, q[2] - q[1], q[0] - q[2]]
        n, m = _cross(p[1], p[2]), _cross(e1, e2)
        Ls = [n, m] + [_cross(f[i], g[j]) for j in range(3) for i in range(3)] + [_cross(n, f[i]) for i in range(3)] + [_cross(m, g[j]) for j in range(3)]
        out = np.zeros((len(A), 17), bool)
        for a, L in enumerate(Ls):
            s = [_dot(L, p[j]) for j in range(3)]
            t = [_dot(L, q[j]) for j in range(3)]
            assert L.dtype == dt and s[0].dtype == dt and t[2].dtype == dt
            out[:, a] = (_min3(*t) > _max3(*s)) | (_max3(*t) < _min3(*s))
    return out


def meets(A, v0, e1, e2):
    """The contract for queries A (N, 3, 3) x records (T, 3), in the arrays' own dtype: (N, T) bool, True where no axis separates.  The
    seventeen axes are evaluated on the pairs the coordinate axes leave (each is a pure comparison: the order is free)."""
    out = np.zeros((len(A), len(v0)), bool)
    qi, ti = np.nonzero(~coordinate_axes(A, v0, e1, e2))
    for s in range(0, len(qi), 1 << 18):
        a, b = qi[s:s + (1 << 18)], ti[s:s + (1 << 18)]
        out[a, b] = ~axes17(A[a], v0[b], e1[b], e2[b]).any(1)
    return out


def meets32(queries, tris):
    """(N, T) bool for (N, 12) query rows over (T, 3, 3) float32 triangles in global id order: the float32 answer (skip not applied)"""
    v0, e1, e2 = records_of(np.ascontiguousarray(tris, f32))
    return meets(vertices_of(queries), v0, e1, e2)


def meets64(queries, tris):
    """the float64 twin: the same operations on the float32 queries and the float32 VERTICES in double (its edges are exact differences)"""
    v0, e1, e2 = records_of(np.ascontiguousarray(tris, f32).astype(np.float64), np.float64)
    return meets(vertices_of(queries).astype(np.float64), v0, e1, e2)


def which_axes(query_tri, scene_tri, dtype=f32):
    """(a coordinate axis separates, the names of the seventeen axes that separate) for one pair of (3, 3) triangles"""
    A = np.asarray(query_tri, dtype).reshape(1, 3, 3)
    v0, e1, e2 = records_of(np.asarray(scene_tri, dtype).reshape(1, 3, 3), dtype)
    return bool(coordinate_axes(A, v0, e1, e2)[0, 0]), [AXES[i] for i in np.nonzero(axes17(A, v0, e1, e2)[0])[0]]


def degenerate(queries):
    """queries that are not traversed: a non-finite coordinate"""
    return ~np.isfinite(vertices_of(queries)).all((1, 2))


class TriTable(Table):
    """overlap_support's Table for (N, 12) query rows: every pair's answer, the skipped triangle taken out like a masked one"""

    def __init__(self, queries, tris, mask=None):
        self.b = np.ascontiguousarray(queries, f32).reshape(-1, 12)
        self.n, self.t = len(self.b), len(tris)
        self.bad = degenerate(self.b)
        self.meets = meets32(self.b, tris) & ~self.bad[:, None] & (np.arange(self.t)[None] != skips_of(self.b).astype(np.int64)[:, None])
        self.mask = np.ones(self.t, bool) if mask is None else np.asarray(mask, bool)


# ---- the exact test: integers, another method ----
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _vol(a, b, c, d):
    """six times the signed volume of the tetrahedron a b c d"""
    (ux, uy, uz), (vx, vy, vz), (wx, wy, wz) = _sub(b, a), _sub(c, a), _sub(d, a)
    return ux * (vy * wz - vz * wy) - uy * (vx * wz - vz * wx) + uz * (vx * wy - vy * wx)


def _sign(x):
    return (x > 0) - (x < 0)


def _orient2(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _on_segment2(a, b, p):
    return min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def _segments_meet2(a, b, c, d):
    o1, o2, o3, o4 = _sign(_orient2(a, b, c)), _sign(_orient2(a, b, d)), _sign(_orient2(c, d, a)), _sign(_orient2(c, d, b))
    if o1 * o2 < 0 and o3 * o4 < 0:
        return True
    return (o1 == 0 and _on_segment2(a, b, c)) or (o2 == 0 and _on_segment2(a, b, d)) or (o3 == 0 and _on_segment2(c, d, a)) or (o4 == 0 and _on_segment2(c, d, b))


def _inside2(t, p):
    s = [_sign(_orient2(t[i], t[(i + 1) % 3], p)) for i in range(3)]
    return not (min(s) < 0 and max(s) > 0)


def _edge_meets(P, Q, T, normal):
    """the closed segment P Q against the closed triangle T of non-zero area (normal: its integer normal)"""
    dp, dq = _vol(T[0], T[1], T[2], P), _vol(T[0], T[1], T[2], Q)
    if (dp > 0 and dq > 0) or (dp < 0 and dq < 0):
        return False
    if dp == 0 and dq == 0:
        # the edge lies in the triangle's plane: drop the coordinate of the normal's largest component
        drop = max(range(3), key=lambda i: abs(normal[i]))
        keep = [i for i in range(3) if i != drop]
        p2, q2, t2 = (P[keep[0]], P[keep[1]]), (Q[keep[0]], Q[keep[1]]), [(v[keep[0]], v[keep[1]]) for v in T]
        return _inside2(t2, p2) or _inside2(t2, q2) or any(_segments_meet2(p2, q2, t2[i], t2[(i + 1) % 3]) for i in range(3))
    # the line P Q crosses the plane in one point of the segment: inside the triangle where it passes its three edges on one side
    s = [_sign(_vol(P, Q, T[i], T[(i + 1) % 3])) for i in range(3)]
    return not (min(s) < 0 and max(s) > 0)


def exact_meets(T1, T2):
    """Two closed triangles of non-zero area with integer coordinates meet iff an edge of one meets the other"""
    T1, T2 = [tuple(int(x) for x in v) for v in T1], [tuple(int(x) for x in v) for v in T2]
    for S, T in ((T1, T2), (T2, T1)):
        u, v = _sub(T[1], T[0]), _sub(T[2], T[0])
        normal = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        assert any(normal), "a triangle of zero area"
        if any(_edge_meets(S[i], S[(i + 1) % 3], T, normal) for i in range(3)):
            return True
    return False


# ---- the lattice: integer coordinates, |x| <= 8 ----
LATTICE = 8


def lattice_tris(rng, n):
    """n triangles of non-zero area with integer coordinates |x| <= 8: a quarter in z = 0, a quarter in z in {-1, 0, 1}, the rest free"""
    out = []
    while len(out) < n:
        kind = len(out) % 4
        t = rng.integers(-LATTICE, LATTICE + 1, (3, 3))
        if kind == 0:
            t[:, 2] = 0
        elif kind == 1:
            t[:, 2] = rng.integers(-1, 2, 3)
        if np.any(np.cross(t[1] - t[0], t[2] - t[0])):
            out.append(t)
    return np.array(out, np.int64)


@functools.lru_cache(maxsize=None)
def lattice_case():
    """(scene (320, 3, 3) int64, queries (128, 3, 3) int64, the exact (128, 320) answer): 40 960 pairs of non-degenerate triangles.  Every
    intermediate value of the predicate is an integer below 3 * 2^18 (|p|, |q| <= 16 per coordinate; a cross of two such 2^9; a cross of
    that with an edge 2^14; a dot of that with q 3 * 2^18), so float32 is exact."""
    rng = np.random.default_rng(2024)
    scene, queries = lattice_tris(rng, 320), lattice_tris(rng, 128)
    exact = np.array([[exact_meets(q, t) for t in scene] for q in queries], bool)
    return scene, queries, exact


# ---- the cases of the GPU tests; tests/test_overlap_triangles.py asserts without a GPU that each reaches what it is named after ----
def tris_around(rng, centres, edge):
    """one triangle per centre (N, 3), vertices within edge[i] / 2 of it on every axis (edge: scalar or (N,)), rounded to float32"""
    c = np.asarray(centres, np.float64)
    e = np.broadcast_to(np.asarray(edge, np.float64), (len(c),))
    return (c[:, None, :] + (rng.random((len(c), 3, 3)) - 0.5) * e[:, None, None]).astype(f32)


def fill_scale(k):
    """the largest edge of the soup's query triangles for pages of k: larger triangles for the larger pages"""
    return 0.8 if k <= 8 else 1.5


@functools.lru_cache(maxsize=None)
def soup_scene():
    """3 000 triangles of edge 0.2 in the unit cube, 384 centres in and just around it, a size in [0, 1) per query (squared: most are small) and the unit shapes"""
    rng = np.random.default_rng(17)
    tris = soup(rng, 3000, edge=0.2)
    centres = around(rng, tris, 384, 0.05)
    unit = rng.random(384) ** 2
    shapes = (rng.random((384, 3, 3)) - 0.5)
    return tris, centres, unit, shapes


@functools.lru_cache(maxsize=None)
def soup_table(scale):
    """the soup with query triangles of edge unit x scale: from no candidate to far more than a page of them"""
    tris, centres, unit, shapes = soup_scene()
    q = (centres.astype(np.float64)[:, None, :] + shapes * (unit * scale)[:, None, None]).astype(f32)
    return TriTable(queries_of_tris(q), tris)


@functools.lru_cache(maxsize=None)
def far_case():
    """the same kind of soup at coordinates near 4 096: the rounding of fl(v0 + e) and of the frame at A0 dominates"""
    rng = np.random.default_rng(19)
    tris = soup(rng, 2000, edge=0.1, offset=4096.0)
    centres = around(rng, tris, 192, 0.05)
    return tris, TriTable(queries_of_tris(tris_around(rng, centres, rng.random(192) * 0.6)), tris)


@functools.lru_cache(maxsize=None)
def needle_case():
    """needles of aspect 10^4: nearly every query meets their vertex boxes and not them"""
    rng = np.random.default_rng(23)
    tris = needles(rng, 2000, 0.2, 1e4)
    centres = around(rng, tris, 192, 0.05)
    return tris, TriTable(queries_of_tris(tris_around(rng, centres, rng.random(192) * 0.6)), tris)


def contact_case(twice=False):
    """Eight stacked unit quads (z = 0, 0.25, ...; triangle 2 i = (0,0) (1,0) (1,1) covers y <= x of quad i, 2 i + 1 = (0,0) (1,1) (0,1)
    covers y >= x) and query triangles that only touch them, each followed by the same triangle one ulp back, with the ids each meets --
    worked out by hand, not by the predicate.  The coordinates are dyadic and every query's first vertex keeps the frame exact, so that
    touching in the reals is touching in float32.  twice: every scene triangle uploaded a second time (id + 16)."""
    _, tris = stacked_quads(8, 0.25)
    up, down = lambda x: float(np.nextafter(f32(x), f32(np.inf))), lambda x: float(np.nextafter(f32(x), f32(-np.inf)))
    cases = [
        ("a vertex on the corner (1, 0) of quad 2", [(1, 0, 0.5), (2, 0, 0.625), (2, -1, 0.375)], [4]),
        ("... one ulp off in x", [(up(1), 0, 0.5), (2, 0, 0.625), (2, -1, 0.375)], []),
        ("a vertex on the corner (1, 1): both triangles of quad 3", [(1, 1, 0.75), (2, 2, 0.875), (1, 2, 0.625)], [6, 7]),
        ("... one ulp off in y", [(1, up(1), 0.75), (2, 2, 0.875), (1, 2, 0.625)], []),
        ("an edge shared with the edge x = 1 of quad 1, the rest beside it", [(1, 0, 0.25), (1, 1, 0.25), (2, 0.5, 0.375)], [2, 3]),
        ("an edge in the edge x = 1 of quad 4, hanging below", [(1, 0.25, 1.0), (1, 0.75, 1.0), (1, 0.5, 0.875)], [8]),
        ("... one ulp beside it", [(up(1), 0.25, 1.0), (up(1), 0.75, 1.0), (up(1), 0.5, 0.875)], []),
        ("a vertex in the face of quad 5, y < x, from above", [(0.75, 0.25, 1.25), (0.875, 0.25, 1.375), (0.75, 0.375, 1.375)], [10]),
        ("... one ulp above it", [(0.75, 0.25, up(1.25)), (0.875, 0.25, 1.375), (0.75, 0.375, 1.375)], []),
        ("a vertex on the diagonal of quad 6, from below", [(0.5, 0.5, 1.5), (0.5, 0.625, 1.375), (0.625, 0.5, 1.375)], [12, 13]),
        ("... one ulp below it", [(0.5, 0.5, down(1.5)), (0.5, 0.625, 1.375), (0.625, 0.5, 1.375)], []),
        ("coplanar with quad 2 and inside its lower triangle", [(0.5, 0.125, 0.5), (0.875, 0.125, 0.5), (0.875, 0.375, 0.5)], [4]),
        ("coplanar with quad 2 and across its diagonal", [(0.5, 0.25, 0.5), (0.75, 0.25, 0.5), (0.25, 0.75, 0.5)], [4, 5]),
        ("coplanar with quad 2 and around all of it", [(-1, -1, 0.5), (4, -1, 0.5), (-1, 4, 0.5)], [4, 5]),
        ("coplanar with quad 2, beside it", [(1.25, 0.5, 0.5), (2, 0, 0.5), (2, 1, 0.5)], []),
        ("coplanar with quad 2, touching its edge x = 1 in a point", [(1, 0.5, 0.5), (2, 0, 0.5), (2, 1, 0.5)], [4]),
        ("in the parallel plane between quads 2 and 3", [(0.5, 0.25, 0.625), (0.75, 0.25, 0.625), (0.25, 0.75, 0.625)], []),
        ("upright through quads 1 to 6, y < x", [(0.75, 0.25, 0.25), (0.75, 0.375, 1.5), (0.75, 0.125, 1.5)], [2, 4, 6, 8, 10, 12]),
        ("upright through the diagonal of quads 3 and 4", [(0.25, 0.75, 0.625), (0.75, 0.25, 0.625), (0.5, 0.5, 1.125)], [6, 7, 8, 9]),
        ("a point in the face of quad 7, y > x", [(0.25, 0.75, 1.75)] * 3, [15]),
        ("... one ulp below it", [(0.25, 0.75, down(1.75))] * 3, []),
        ("a segment through quads 0 and 1, y > x", [(0.25, 0.5, -0.125), (0.25, 0.5, 0.375), (0.25, 0.5, 0.375)], [1, 3]),
        ("a segment that ends on quad 1", [(0.25, 0.5, 0.25), (0.25, 0.5, 0.375), (0.25, 0.5, 0.375)], [3]),
        ("... one ulp above it", [(0.25, 0.5, up(0.25)), (0.25, 0.5, 0.375), (0.25, 0.5, 0.375)], []),
        ("everything", [(0.5, 0.5, -1), (0.5, 0.5, 3), (0.5, 0.5625, 3)], list(range(16))),
        ("beside everything", [(1.5, 1.5, 0), (2, 2, 2), (2, 1.5, 1)], []),
    ]
    if twice:
        tris = np.concatenate([tris, tris])
        cases = [(name, q, ids + [g + 16 for g in ids]) for name, q, ids in cases]
    return tris, [c[0] for c in cases], queries_of_tris(np.array([c[1] for c in cases], f32)), [c[2] for c in cases]


def spiral_queries(n, seed=6160):
    """The queries of the deep-tree test on deep_tree_support.spiral(n), fixed by the seed: thin triangles from the origin, whose
    neighbourhood every triangle's vertex box contains -- they keep both children at every level --, along the spiral's axis -(1, 1, 1),
    of lengths that reach none of the triangles, only the innermost, half of the chain and all of it; a thin triangle inside each triangle
    of the spiral, from its centroid to its first vertex; thin triangles beside everything; and queries that are not traversed."""
    from deep_tree_support import scales, spiral
    rng = np.random.default_rng(seed + n)
    s = scales(n)
    tris = spiral(n).astype(np.float64)
    q = []
    for size in (0.01 * s[0], 0.3 * s[0], s[2], s[n // 2], s[n - 4], 3.0 * s[-1]):
        for _ in range(12):
            # triangle k lies in the plane x + y + z = -s_k / 2 and holds the foot of the origin well inside: a thin triangle from the
            # origin along -(1, 1, 1) of length `size` passes through the triangles with s_k < 3.46 size
            a = rng.uniform(-1, 1, 3) * 0.01 * s[0]
            d = np.ones(3) / np.sqrt(3.0) + rng.normal(size=3) * 0.01
            d *= size / np.linalg.norm(d)
            q.append([a, a - d, a - d + np.cross(d, rng.normal(size=3)) * 0.01])
    cen = tris.mean(1)
    for g in range(n):
        q.append([cen[g], tris[g, 0], tris[g, 0] + (tris[g, 1] - tris[g, 0]) * 0.02])
        q.append([cen[g] * 3.0 + s[g], cen[g] * 3.0 + 1.1 * s[g], cen[g] * 3.0 + 1.05 * s[g]])
    q = np.array(q, f32)
    bad = np.array([[(np.nan, 0, 0), (1, 1, 1), (0, 1, 0)], [(0, 0, 0), (1, np.inf, 1), (0, 1, 0)], [(0, 0, 0), (1, 1, 1), (0, 1, -np.inf)]], f32)
    return queries_of_tris(np.concatenate([q, bad]))
