"""Helpers of the winding-number tests (cap_winding_build, cap_winding_numbers): the float64 dipole table of include/capsaicin_hip.h
("winding numbers") from a read-back tree, the walk of the query restated on the host -- the far / near decisions in float32 exactly as
the header writes them, the terms in float64 (walk) or in the device's float32 form (walk32) --, a median-split tree in
cap_bvh_readback's format so that the CPU tests run the same walk code, and the open test meshes.  Ground truth is the float64 brute
force signed_distance_support.winding_number."""
import functools

import numpy as np

from closest_point_support import around, closest, queries, sphere
from refit_support import padded_boxes
from signed_distance_support import MESHES, box, mesh, truth_case, winding_number  # noqa: F401  (winding_number: the tests' ground truth)

f32 = np.float32
LEAF_SHIFT, LEAF_MASK = 27, (1 << 27) - 1
K4PI, KINV2PI = f32(12.566371), f32(0.15915494)  # fl(4 pi), fl(1 / (2 pi)): the kernel's constants


def children(nodes):
    """(inner nodes, 2) int32: the traversal child codes, words 14 and 15 of cap_bvh_readback's nodes"""
    return np.ascontiguousarray(np.asarray(nodes, f32).reshape(-1, 16)[:, 14:16]).view(np.int32)


def leaf_range(code):
    c = ~int(code) & 0xFFFFFFFF
    first = c & LEAF_MASK
    return first, first + (c >> LEAF_SHIFT) + 1


def root_code(n_tris):
    return 0 if n_tris >= 2 else -1  # ~0: the one triangle


def child_boxes(nodes):
    """(inner nodes, 2, 2, 3) float32: per slot (lo, hi) of the child's stored box"""
    return np.asarray(nodes, f32).reshape(-1, 16)[:, 0:12].reshape(-1, 2, 2, 3)


# ---- the table, float64 ----
def triangle_sums(tris):
    """(T, 7) float64 (n_t, a_t, a_t c_t) of (T, 3, 3) float32 triangles and the mask of the live ones"""
    P = np.asarray(tris, f32).astype(np.float64).reshape(-1, 3, 3)
    finite = np.isfinite(P).all((1, 2))
    with np.errstate(all="ignore"):
        e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        n = 0.5 * np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        a = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        c = ((P[:, 0] + P[:, 1]) + P[:, 2]) / 3.0
    live = finite & (n != 0).any(1)
    s = np.zeros((len(P), 7))
    s[live, 0:3], s[live, 3], s[live, 4:7] = n[live], a[live], a[live, None] * c[live]
    return s, live


def moments(nodes, order, tris):
    """The float64 table of a read-back tree: (table (inner nodes, 2, 8) float64 = p~, r, N, the child code as a number; info dict,
    with the slots' areas A as "areas").
    p~ and N are not yet rounded; r is measured from the float32-rounded p~, as the definition says, not yet rounded or stepped."""
    nodes = np.asarray(nodes, f32).reshape(-1, 16)
    order = np.asarray(order).astype(np.int64)
    kid, boxes = children(nodes), child_boxes(nodes).astype(np.float64)
    per_tri, live = triangle_sums(np.asarray(tris, f32).reshape(-1, 3, 3)[order])
    memo = {}

    def sums(code):
        code = int(code)
        if code not in memo:
            if code < 0:
                first, end = leaf_range(code)
                s = np.zeros(7)
                for t in range(first, end):
                    s = s + per_tri[t]
            else:
                s = sums(kid[code, 0]) + sums(kid[code, 1])
            memo[code] = s
        return memo[code]

    table, areas = np.zeros((len(nodes), 2, 8)), np.zeros((len(nodes), 2))
    for i in range(len(nodes)):
        for s in range(2):
            m = sums(kid[i, s])
            lo, hi = boxes[i, s]
            p = m[4:7] / m[3] if m[3] != 0 else 0.5 * (lo + hi)
            p32 = p.astype(f32).astype(np.float64)
            d = np.maximum(np.abs(lo - p32), np.abs(hi - p32))
            table[i, s, 0:3], table[i, s, 3], table[i, s, 4:7], table[i, s, 7] = p, np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), m[0:3], kid[i, s]
            areas[i, s] = m[3]
    total = sums(root_code(len(order))) if len(order) else np.zeros(7)
    info = dict(inner_nodes=len(nodes), degenerate_triangles=int(len(order) - live.sum()), total_area=float(total[3]), root_n=total[0:3].copy(),
                root_p=(total[4:7] / total[3] if total[3] != 0 else None), areas=areas)
    return table, info


def table32_of(table64):
    """the (inner nodes, 2, 8) float32 table the device would store for a float64 one: p~ and N rounded once, r rounded and stepped
    one ulp up, word 7 the child code's bits"""
    t = np.zeros(table64.shape, f32)
    t[:, :, 0:3], t[:, :, 4:7] = table64[:, :, 0:3], table64[:, :, 4:7]
    t[:, :, 3] = np.nextafter(table64[:, :, 3].astype(f32), f32(np.inf))
    t.view(np.int32)[:, :, 7] = table64[:, :, 7].astype(np.int64).astype(np.int32)
    return t


# ---- the walk ----
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _records32(tris, order):
    """(v0, e1, e2, n) of the stored intersection records in leaf order, float32: n = cross(e1, e2), every operation rounded"""
    t = np.asarray(tris, f32).reshape(-1, 3, 3)[np.asarray(order).astype(np.int64)]
    v0, e1, e2 = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    with np.errstate(all="ignore"):
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    assert n.dtype == f32
    return v0, e1, e2, n


def _exact64(q, tri):
    """Van Oosterom & Strackee in float64 on the triangle's vertices: signed_distance_support.winding_number's term for points q (K, 3)"""
    a, b, c = (tri[k][None] - q for k in range(3))
    la, lb, lc = (np.sqrt((x * x).sum(1)) for x in (a, b, c))
    num = (a * np.cross(b, c)).sum(1)
    den = la * lb * lc + (a * b).sum(1) * lc + (b * c).sum(1) * la + (c * a).sum(1) * lb
    return 2.0 * np.arctan2(num, den) / (4.0 * np.pi)


def _exact32(q, v0, e1, e2, n):
    """the kernel's float32 form on one stored record for points q (K, 3) float32"""
    a = v0[None] - q
    b, c = a + e1[None], a + e2[None]
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    det = _dot(a, n[None])
    den = (((la * lb) * lc + _dot(a, b) * lc) + _dot(b, c) * la) + _dot(c, a) * lb
    t = np.arctan2(det, den) * KINV2PI
    assert t.dtype == f32
    return t


def _walk(nodes, order, tris, table32, points, beta, single):
    q32 = np.ascontiguousarray(np.asarray(points, f32)[:, 0:3])
    q64 = q32.astype(np.float64)
    N, T = len(q32), len(order)
    acc, visits = np.zeros(N), np.zeros((N, 2), np.int64)
    ok = np.isfinite(q32).all(1)
    table32 = np.asarray(table32, f32).reshape(-1, 2, 8)
    codes = table32.view(np.int32)[:, :, 7]
    t64 = np.asarray(tris, f32).astype(np.float64).reshape(-1, 3, 3)[np.asarray(order).astype(np.int64)]
    rec = _records32(tris, order) if single else None
    beta = f32(beta)
    stack = [(root_code(T), np.nonzero(ok)[0])] if T else []
    with np.errstate(all="ignore"):
        while stack:
            code, idx = stack.pop()
            if len(idx) == 0:
                continue
            if code < 0:
                first, end = leaf_range(code)
                for t in range(first, end):
                    if single:
                        term = _exact32(q32[idx], rec[0][t], rec[1][t], rec[2][t], rec[3][t]).astype(np.float64)
                    else:
                        term = _exact64(q64[idx], t64[t])
                    acc[idx] += np.where(np.isnan(term), 0.0, term)
                visits[idx, 1] += end - first
                continue
            near = []
            for s in range(2):
                p, r, nn = table32[code, s, 0:3], table32[code, s, 3], table32[code, s, 4:7]
                d = p[None] - q32[idx]
                d2 = _dot(d, d)
                lim = beta * r
                far = d2 > lim * lim
                assert d2.dtype == f32 and np.asarray(lim).dtype == f32
                if single:
                    term = (_dot(nn[None], d) / ((K4PI * d2) * np.sqrt(d2))).astype(np.float64)
                else:
                    d64 = p.astype(np.float64)[None] - q64[idx]
                    l2 = (d64 * d64).sum(1)
                    term = (nn.astype(np.float64)[None] * d64).sum(1) / (4.0 * np.pi * l2 * np.sqrt(l2))
                acc[idx[far]] += term[far]
                visits[idx[far], 0] += 1
                near.append(idx[~far])
            # slot 0's subtree before slot 1's: slot 1 waits on the stack
            stack.append((int(codes[code, 1]), near[1]))
            stack.append((int(codes[code, 0]), near[0]))
    acc[~ok] = np.nan
    return acc, visits


def walk(nodes, order, tris, table32, points, beta):
    """(w (N,) float64, visits (N, 2)) of cap_winding_numbers' walk over the read-back tree and float32 table: the far / near test in
    float32 exactly as specified, the terms in float64 on the original vertices, added in the kernel's order"""
    return _walk(nodes, order, tris, table32, points, beta, False)


def walk32(nodes, order, tris, table32, points, beta):
    """the same walk with every term in the kernel's float32 arithmetic, widened and added into a float64 accumulator"""
    return _walk(nodes, order, tris, table32, points, beta, True)


# ---- a tree for the CPU tests ----
def median_tree(tris, leaf=4):
    """(nodes (T - 1, 16) float32, order (T,) uint32) in cap_bvh_readback's format: a complete binary tree by median splits of the
    centroids along the longest axis, child boxes the unions of the padded triangle boxes, words 12 and 13 the binary children, words
    14 and 15 the traversal children with a subtree of at most `leaf` triangles as one leaf code"""
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    T = len(tris)
    plo, phi = padded_boxes(tris)
    cen = tris.astype(np.float64).mean(1)
    nodes = np.zeros((max(T - 1, 0), 16), f32)
    kid = nodes.view(np.int32)
    order = np.zeros(T, np.uint32)
    counter = [0, 0]  # next node, next leaf position

    def build(ids):
        """returns (binary code, traversal code, lo, hi) of the subtree over ids; leaves take the next positions of the order"""
        if len(ids) == 1:
            pos = counter[1]
            counter[1] += 1
            order[pos] = ids[0]
            return ~pos, ~pos, plo[ids[0]], phi[ids[0]]
        me = counter[0]
        counter[0] += 1
        first = counter[1]
        c = cen[ids]
        axis = int(np.argmax(c.max(0) - c.min(0)))
        ids = ids[np.argsort(c[:, axis], kind="stable")]
        half = len(ids) // 2
        out = [build(ids[:half]), build(ids[half:])]
        for s, (bc, tc, lo, hi) in enumerate(out):
            nodes[me, 6 * s:6 * s + 3], nodes[me, 6 * s + 3:6 * s + 6] = lo, hi
            kid[me, 12 + s], kid[me, 14 + s] = bc, tc
        tcode = ~(first | ((len(ids) - 1) << LEAF_SHIFT)) if len(ids) <= leaf else me
        return me, tcode, np.minimum(out[0][2], out[1][2]), np.maximum(out[0][3], out[1][3])

    if T >= 2:
        build(np.arange(T))
    elif T == 1:
        order[0] = 0
    return nodes, order


# ---- meshes ----
def open_cube():
    """the unit cube wound outwards, less its top face (z = 1): 10 triangles; w = 5/6 at the centre"""
    t = box((1.0, 1.0, 1.0))
    keep = ~(t[:, :, 2] == 1.0).all(1)
    assert keep.sum() == 10
    return np.ascontiguousarray(t[keep])


def punctured(mesh, k, seed=11):
    """(the mesh less k of its triangles, chosen by the seed; the removed triangles): k holes of one triangle each"""
    rng = np.random.default_rng(seed)
    gone = np.sort(rng.choice(len(mesh), k, replace=False))
    keep = np.ones(len(mesh), bool)
    keep[gone] = False
    return np.ascontiguousarray(mesh[keep]), np.ascontiguousarray(mesh[gone])


def octant_triangle(flip=False):
    """(1,0,0), (0,1,0), (0,0,1): an eighth of the sphere seen from the origin.  As wound here its normal (1,1,1) points away from the
    origin, the way an outward-wound mesh around the origin would: w = +1/8 there, -1/8 flipped"""
    t = f32([[(1, 0, 0), (0, 1, 0), (0, 0, 1)]])
    return t[:, [0, 2, 1]] if flip else t


def unit_sphere():
    return sphere(50, 50)


def overflow_scene():
    """two triangles with edges of 1e10 near the origin, both normals along +x, so that the root is an inner node with |N| = 5e19 per
    slot; and three points: one whose d2 overflows to +inf and whose dot(N, d) overflows (the far term is inf / inf), one far with a
    finite d2, one near both triangles"""
    t = np.float32([[(0, 0, 0), (0, 1e10, 0), (0, 0, 1e10)]])
    tris = np.concatenate([t, (t + np.float32([2e9, 3e9, -1e9])).astype(np.float32)])
    return tris, queries(np.float32([(3e19, 0, 0), (1e15, 0, 0), (5e9, 3e9, 3e9)]))


# ---- the query cases the CPU and GPU tests share ----
OPEN_MESHES = {
    "open cube": open_cube,
    "punctured sphere": lambda: punctured(unit_sphere(), 8)[0],
    "octant triangle": octant_triangle,
}
BETAS = (2.0, 4.0, np.inf)


@functools.lru_cache(maxsize=None)
def query_case(name):
    """(triangles, kept points (K, 4) float32, inside flags or None, kept share of the drawn points): every fourth kept point of
    signed_distance_support.truth_case for its closed meshes; for the open ones 1 000 points in the box grown by 0.3 (seed 7), kept
    by the same rule, at least 10^-3 of the box diagonal off the surface"""
    if name in MESHES:
        tris = mesh(name)
        q, _, inside, keep = truth_case(name)
        pts, share, inside = q[keep][::4], len(keep) / len(q), inside[::4]
    else:
        tris = OPEN_MESHES[name]()
        q = queries(around(np.random.default_rng(7), tris, 1000, 0.3))
        rec, _ = closest(q, tris)
        v = tris.reshape(-1, 3).astype(np.float64)
        keep = np.sqrt(rec[:, 3].astype(np.float64)) >= 1e-3 * np.linalg.norm(v.max(0) - v.min(0))
        pts, share, inside = q[keep], keep.mean(), None
    pts = np.ascontiguousarray(pts, f32)
    for a in (tris, pts):
        a.setflags(write=False)
    return tris, pts, inside, float(share)
