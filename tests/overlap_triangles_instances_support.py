"""Helpers of the instanced triangle overlap tests (cap_overlap_triangles_instances): the float32 brute force --
closest_instances_support.world_records for the world record of every (instance, triangle), overlap_triangles_support.meets for the
17-axis predicate on it --, the pair table (overlap_instances_support.PairTable's candidates / page / counts / pages under the (i, g)
cursor) with valid pairs and the skip pair, a numpy model of the world-node prune with the constant as a parameter, the wrapper of
cap_debug_overlap_world_node, and the case builders of the GPU tests."""
import ctypes as C
import functools

import numpy as np

from closest_instances_support import affine, identity, near_translations, pair_valid, world_records  # noqa: F401
from closest_point_support import needles, soup
from instance_support import regular_transforms
from overlap_instances_support import (C2, EPS32, MISS, PairTable, all_miss, assert_counts, assert_pair_pages, cursors_of, fill_classes,  # noqa: F401
                                       model_image, model_miss, pages)
from overlap_support import ids_of  # noqa: F401
from overlap_triangles_support import NONE, contact_case, degenerate, meets, queries_of, queries_of_tris, skips_of, vertices_of  # noqa: F401

f32 = np.float32


def skip_instances_of(queries):
    """the pad0 word of (N, 12) rows, which this call reads as skip_instance"""
    return np.ascontiguousarray(queries, f32).reshape(-1, 12).view(np.uint32)[:, 7].copy()


def with_skip_pair(queries, instances, ids):
    """a copy of the rows with the skip pair set to (instances, ids)"""
    q = np.ascontiguousarray(queries, f32).reshape(-1, 12).copy()
    q.view(np.uint32)[:, 3] = np.asarray(ids, np.int64).astype(np.uint32)
    q.view(np.uint32)[:, 7] = np.asarray(instances, np.int64).astype(np.uint32)
    return q


def meets_pairs(queries, M, tris, dtype=np.float32, chunk=64):
    """(N, I * T) bool: the contract's predicate on the world record of every pair, flat index i * T + g (the skip pair not applied).
    dtype=float64 is the twin: the same operations on the float32 queries, transforms and vertices in double."""
    A = vertices_of(queries).astype(dtype)
    M = np.asarray(M, f32).reshape(-1, 3, 4)
    v0w, e1w, e2w = (x.reshape(-1, 3) for x in world_records(M, np.ascontiguousarray(tris, f32), dtype))
    out = np.zeros((len(A), len(v0w)), bool)
    for s in range(0, len(A), chunk):
        out[s:s + chunk] = meets(A[s:s + chunk], v0w, e1w, e2w)
    return out


class TriPairTable(PairTable):
    """PairTable for (N, 12) world-space query rows over (T, 3, 3) triangles under (I, 3, 4) transforms: every pair's answer, the
    skip pair (pad0, skip) taken out like a masked pair.  valid: (I, T) bool from pair_valid, None = every pair."""

    def __init__(self, queries, M, tris, valid=None):
        self.b = np.ascontiguousarray(queries, f32).reshape(-1, 12)
        M = np.asarray(M, f32).reshape(-1, 3, 4)
        self.n, self.i, self.t = len(self.b), len(M), len(tris)
        self.bad = degenerate(self.b)
        self.inst_of, self.tri_of = np.divmod(np.arange(self.i * self.t, dtype=np.int64), self.t)
        self.meets = meets_pairs(self.b, M, tris) & ~self.bad[:, None]
        g, i = skips_of(self.b).astype(np.int64), skip_instances_of(self.b).astype(np.int64)
        own = np.nonzero((g < self.t) & (i < self.i))[0]  # (an id of ~0, or a pair beyond the table, skips nothing)
        self.meets[own, i[own] * self.t + g[own]] = False
        self.valid = np.ones(self.i * self.t, bool) if valid is None else np.asarray(valid, bool).reshape(-1)

    def pairs(self, q, cursor=None):
        return [(int(self.inst_of[f]), int(self.tri_of[f])) for f in self.candidates(q, cursor)]


# ---- the prune: the debug entry, and the same arithmetic in numpy with the constant as a parameter ----
def world_node(M, object_lo, object_hi, node_lo, node_hi, query_lo, query_hi, lib=None):
    """cap_debug_overlap_world_node: {xw, slack, world_lo, world_hi, skip_node}"""
    if lib is None:
        from capsaicin_amd import capi
        lib = capi.lib()
    f3 = C.c_float * 3
    v = lambda x: f3(*np.asarray(x, f32).reshape(3).tolist())
    m = (C.c_float * 12)(*np.asarray(M, f32).reshape(12).tolist())
    wlo, whi = f3(), f3()
    xw, slack, node = C.c_float(), C.c_float(), C.c_uint32()
    rc = lib.cap_debug_overlap_world_node(m, v(object_lo), v(object_hi), v(node_lo), v(node_hi), v(query_lo), v(query_hi), C.byref(xw), C.byref(slack),
                                          wlo, whi, C.byref(node))
    assert rc == 0, lib.cap_last_error()
    return dict(xw=xw.value, slack=slack.value, world_lo=np.array(wlo[:], f32), world_hi=np.array(whi[:], f32), skip_node=int(node.value))


def model_world_box(M, node_lo, node_hi):
    """cap_near.h overlap_world_box in float32 numpy, one rounded operation per operation there: the world (lo, hi) of object-space
    boxes (..., 3) under the transform M (3, 4)"""
    M, lo, hi = np.asarray(M, f32).reshape(3, 4), np.asarray(node_lo, f32), np.asarray(node_hi, f32)
    with np.errstate(all="ignore"):
        hl, hh = lo * f32(0.5), hi * f32(0.5)
        c, h = hl + hh, hh - hl
        A = np.abs(M)
        cw = np.stack([((M[r, 0] * c[..., 0] + M[r, 1] * c[..., 1]) + M[r, 2] * c[..., 2]) + M[r, 3] for r in range(3)], -1)
        hw = np.stack([(A[r, 0] * h[..., 0] + A[r, 1] * h[..., 1]) + A[r, 2] * h[..., 2] for r in range(3)], -1)
        assert cw.dtype == f32 and hw.dtype == f32
        return cw - hw, cw + hw


def model_world_skip(M, xw, node_lo, node_hi, query_lo, query_hi, c2=C2):
    """the model of world_node_step's test: True where the node's world box misses the query box grown by c2 eps (|query box|_inf + xw)"""
    qlo, qhi = np.asarray(query_lo, f32), np.asarray(query_hi, f32)
    wlo, whi = model_world_box(M, node_lo, node_hi)
    with np.errstate(all="ignore"):
        bmax = np.maximum(np.abs(qlo), np.abs(qhi)).max(-1)
        slack = ((f32(c2) * EPS32) * (bmax + f32(xw)))[..., None]
        assert slack.dtype == f32
        return model_miss(wlo, whi, qlo - slack, qhi + slack)


LEAF_SHIFT, LEAF_MASK = 27, (1 << 27) - 1


def world_walk(nodes, order, M, xw, query_lo, query_hi):
    """k_overlap_tri_inst's walk of one instance for one query box over the host builder's tree (nodes (N, 16) float32: child 0's lo and
    hi, child 1's, two words, the children; order: leaf slot -> triangle): a child is kept unless the model of world_node_step skips it;
    both kept -> child 0 is entered and child 1 pushed.  Returns (the stack's high-water mark, the triangles of the leaves reached)."""
    kid = np.ascontiguousarray(nodes[:, 14:16]).view(np.int32)
    stack, high, reached, node = [], 0, [], 0
    while True:
        if node >= 0:
            q = nodes[node]
            k0 = not model_world_skip(M, xw, q[0:3], q[3:6], query_lo, query_hi)
            k1 = not model_world_skip(M, xw, q[6:9], q[9:12], query_lo, query_hi)
            c0, c1 = int(kid[node, 0]), int(kid[node, 1])
            if k0 and k1:
                stack.append(c1)
                high = max(high, len(stack))
                node = c0
                continue
            if k0 or k1:
                node = c0 if k0 else c1
                continue
        else:
            code = ~int(node) & 0xFFFFFFFF
            first = code & LEAF_MASK
            reached += [int(order[l]) for l in range(first, first + (code >> LEAF_SHIFT) + 1)]
        if not stack:
            break
        node = stack.pop()
    return high, reached


def query_boxes(queries):
    """(min, max) of the vertices of (N, 12) rows, each (N, 3): what the walk prunes against"""
    A = vertices_of(queries)
    with np.errstate(invalid="ignore"):
        return A.min(1), A.max(1)


# ---- the cases of the GPU tests; tests/test_overlap_triangles_instances.py asserts without a GPU that each reaches what it is named after ----
def queries_near(rng, M, tris, n, size=0.3, away=8):
    """n world-space query triangles around random world points of random triangles of random instances, vertices within
    rng^2 x size x the instance's scale ||L||_F / sqrt 3 of the point (most are small, some reach many triangles); every `away`-th is
    moved off by three scales (most of those meet nothing)"""
    Md = np.asarray(M, f32).astype(np.float64)
    i, g = rng.integers(0, len(Md), n), rng.integers(0, len(tris), n)
    x = np.einsum("nk,nkj->nj", rng.dirichlet((1, 1, 1), n), np.asarray(tris, np.float64)[g])
    y = np.einsum("nrk,nk->nr", Md[i][:, :, :3], x) + Md[i][:, :, 3]
    scale = np.linalg.norm(Md[i][:, :, :3], axis=(1, 2)) / np.sqrt(3.0)
    edge = rng.random(n) ** 2 * size * scale
    v = y[:, None, :] + (rng.random((n, 3, 3)) - 0.5) * 2.0 * edge[:, None, None]
    v[::away] += 3.0 * scale[::away, None, None]
    return queries_of_tris(v.astype(f32))


def soup_transforms():
    """regular_transforms(32) with four of them copies of another one (two exact, two moved by a hundredth of their size) so that
    pages span instances"""
    M = regular_transforms(32).copy()
    for j in (5, 12, 20, 27):
        M[j] = M[j - 4]
    for j in (20, 27):
        M[j, :, 3] += f32(0.01) * np.abs(M[j, :, :3]).max()
    return M


@functools.lru_cache(maxsize=None)
def soup_case():
    """600 triangles under the 32 transforms of soup_transforms(); 512 queries: (triangles, transforms, table)"""
    tris = soup(np.random.default_rng(3), 600, edge=0.2)
    M = soup_transforms()
    return tris, M, TriPairTable(queries_near(np.random.default_rng(31), M, tris, 512, size=1.8), M, tris)


@functools.lru_cache(maxsize=None)
def regular_case():
    """the soup under regular_transforms(32) as they are"""
    tris = soup(np.random.default_rng(3), 600, edge=0.2)
    M = regular_transforms(32)
    return tris, M, TriPairTable(queries_near(np.random.default_rng(34), M, tris, 512, size=1.0), M, tris)


@functools.lru_cache(maxsize=None)
def far_case():
    """the soup with the translations near 4 096: the world record's rounding of 2^-12 against triangles of size 0.2"""
    tris = soup(np.random.default_rng(3), 600, edge=0.2)
    M = near_translations(regular_transforms(32))
    return tris, M, TriPairTable(queries_near(np.random.default_rng(32), M, tris, 512, size=1.0), M, tris)


@functools.lru_cache(maxsize=None)
def needle_case():
    """needles of aspect 10^4 under 16 transforms: nearly every query meets their vertex boxes and not them"""
    tris = needles(np.random.default_rng(12), 600, 0.2, 1e4)
    M = regular_transforms(16)
    return tris, M, TriPairTable(queries_near(np.random.default_rng(33), M, tris, 512, size=1.0), M, tris)


def odd_queries():
    """far and non-finite queries (the first four are traversed)"""
    nan, inf = np.nan, np.inf
    t = [[(-1e30, -1e30, -1e30), (1e30, 1e30, 1e30), (1e30, -1e30, 0)], [(1e20, 1e20, 1e20), (1e20, 1.1e20, 1e20), (1.1e20, 1e20, 1e20)],
         [(0, 0, 0), (0, 0, 0), (0, 0, 0)], [(-1e18, 0.25, 0.5), (1e18, 0.75, 0.5), (1e18, 0.75, 0.5)],
         [(nan, 0, 0), (1, 1, 1), (0, 1, 0)], [(0, 0, 0), (1, inf, 1), (0, 1, 0)], [(0, 0, 0), (1, 1, 1), (0, 1, -inf)], [(nan,) * 3] * 3]
    return queries_of_tris(np.array(t, f32))


def contact_instances():
    """contact_case()'s quads under a power-of-two translation and under diag(2, 1, 1): (triangles, transforms, names, world queries, the
    (instance, triangle) pairs each meets, worked out by hand): instance 0's queries are the case's moved by the translation,
    instance 1's the case's with x doubled and moved -- both maps are exact on the dyadic coordinates, and the images lie too far apart
    to meet each other's quads.  A coordinate the case moved one ulp off a dyadic value is one ulp of its IMAGE off again, on the same
    side."""
    tris, names, q, want = contact_case()
    t = np.array([64.0, -32.0, 16.0])
    M = np.stack([affine(np.eye(3), t), affine(np.diag([2.0, 1.0, 1.0]), (-64.0, 0.0, 0.0))])
    A = vertices_of(q).astype(np.float64)

    def image(scale, move):
        x = A * scale + move  # (exact in double)
        r = x.astype(f32)
        r = np.where(x > r, np.nextafter(r, f32(np.inf)), np.where(x < r, np.nextafter(r, f32(-np.inf)), r))
        return queries_of_tris(r)

    q0, q1 = image(np.ones(3), t), image(np.array([2.0, 1.0, 1.0]), np.array([-64.0, 0.0, 0.0]))
    pairs = [[(0, g) for g in ids] for ids in want] + [[(1, g) for g in ids] for ids in want]
    return tris, M, ["translated: " + n for n in names] + ["stretched: " + n for n in names], np.concatenate([q0, q1]), pairs


def counterexample():
    """The scene that defeats cap_overlap_instances' bottom-level prune for the triangle predicate: instance 0 is a rotation by 45
    degrees about z, instance 1 the identity; triangle 0 is a segment (b = c) whose image under instance 0 runs from (-3, 1, 0) to
    (1, -3, 0), followed by 63 small filler triangles at least 10 units away from it; the query is the segment (0, 0, 0) - (1, 1, 0).
    The two segments are coplanar and do not cross, which the 17 axes cannot decide: the pair (0, 0) is a candidate by the contract.
    (triangles (64, 3, 3), transforms (2, 3, 4), the query row)"""
    c = np.sqrt(0.5)
    R = np.array([[c, -c, 0.0], [c, c, 0.0], [0.0, 0.0, 1.0]])
    world = np.array([(-3.0, 1.0, 0.0), (1.0, -3.0, 0.0)])
    seg = (world @ R).astype(f32)  # object-space vertices: R^T w, row by row
    rng = np.random.default_rng(77)
    # two groups on the far side of the segment from the query's image, so that whichever way a builder splits them every box above
    # the segment stays on that side
    centres = np.stack([np.where(np.arange(63) < 40, -14.0, -60.0) + 2.0 * rng.random(63), -3.0 + 6.0 * rng.random(63), -0.5 + rng.random(63)], 1)
    filler = (centres[:, None, :] + (rng.random((63, 3, 3)) - 0.5) * 0.2).astype(f32)
    tris = np.concatenate([np.stack([seg[0], seg[1], seg[1]])[None], filler])
    M = np.stack([affine(R), identity()[0]])
    return tris, M, queries_of([(0, 0, 0)], [(1, 1, 0)], [(1, 1, 0)])
