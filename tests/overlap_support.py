"""Helpers of the box overlap tests (cap_overlap_boxes): the 13-axis predicate of include/capsaicin_hip.h transcribed to numpy, vectorised
over boxes x triangles -- one rounded operation per operation of the contract, float32 throughout on the answer path (the same code runs
in float64 as the twin it is judged against) --, the boxes that are not traversed, a box's candidates under mask and cursor in id order,
the expected (N, k) pages and counts, pages(), which applies the cursor rule until nothing is left, and the model walker of the deep-tree
test."""
import copy
import functools

import numpy as np

from closest_point_support import around, needles, records_of, soup
from multi_hit_support import stacked_quads

MISS = 0xFFFFFFFF
f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
X, Y, Z = 0, 1, 2


def boxes_of(lo, hi):
    """(N, 8) float32 CapBoxDesc rows of (N, 3) corners; the pad words hold a NaN, which nobody may read"""
    lo, hi = np.asarray(lo, f32).reshape(-1, 3), np.asarray(hi, f32).reshape(-1, 3)
    b = np.full((len(lo), 8), np.nan, f32)
    b[:, 0:3], b[:, 4:7] = lo, hi
    return b


def _min3(a, b, c):
    return np.minimum(np.minimum(a, b), c)  # (hands a NaN on)


def _max3(a, b, c):
    return np.maximum(np.maximum(a, b), c)


def meets(lo, hi, v0, e1, e2):
    """The contract for boxes (N, 3) x records (T, 3), in the arrays' own dtype: (N, T) bool, True where no axis separates"""
    by_box, by_cross, by_plane = axes(lo, hi, v0, e1, e2)
    return ~(by_box | by_cross | by_plane)


def axes(lo, hi, v0, e1, e2):
    """(N, T) bool each: a box axis separates, one of the nine cross axes does, the triangle's plane does.  Every axis is evaluated for
    every pair (they are pure comparisons)."""
    dt = lo.dtype
    assert hi.dtype == dt and v0.dtype == dt and e1.dtype == dt and e2.dtype == dt
    half = dt.type(0.5)
    with np.errstate(all="ignore"):
        lo, hi = lo[:, None, :], hi[:, None, :]
        a, b, c = v0[None], (v0 + e1)[None], (v0 + e2)[None]
        # 1. the box axes, absolute coordinates
        by_box = ((_min3(a, b, c) > hi) | (_max3(a, b, c) < lo)).any(-1)
        by_cross = np.zeros(by_box.shape, bool)
        # 2. the centred frame
        hl, hh = lo * half, hi * half
        ctr, h = hl + hh, hh - hl
        P = [a - ctr, b - ctr, c - ctr]
        F = [np.broadcast_to(e1[None], P[0].shape), P[2] - P[1], P[0] - P[2]]
        # 3. the nine cross axes
        for f in F:
            af = np.abs(f)
            for m, n in ((Y, Z), (Z, X), (X, Y)):
                s = [f[..., m] * p[..., n] - f[..., n] * p[..., m] for p in P]
                r = h[..., m] * af[..., n] + h[..., n] * af[..., m]
                by_cross |= (_min3(*s) > r) | (_max3(*s) < -r)
        # 4. the triangle's plane
        nx = e1[:, Y] * e2[:, Z] - e1[:, Z] * e2[:, Y]
        ny = e1[:, Z] * e2[:, X] - e1[:, X] * e2[:, Z]
        nz = e1[:, X] * e2[:, Y] - e1[:, Y] * e2[:, X]
        d = (nx * P[0][..., X] + ny * P[0][..., Y]) + nz * P[0][..., Z]
        r = (h[..., X] * np.abs(nx) + h[..., Y] * np.abs(ny)) + h[..., Z] * np.abs(nz)
        by_plane = (d > r) | (d < -r)
        assert d.dtype == dt and r.dtype == dt and P[0].dtype == dt
    return by_box, by_cross, by_plane


def meets32(boxes, tris, chunk=256):
    """(N, T) bool for (N, 8) box rows over (T, 3, 3) float32 triangles in global id order: the float32 answer"""
    b = np.ascontiguousarray(boxes, f32).reshape(-1, 8)
    v0, e1, e2 = records_of(np.ascontiguousarray(tris, f32))
    out = np.zeros((len(b), len(v0)), bool)
    for s in range(0, len(b), chunk):
        out[s:s + chunk] = meets(b[s:s + chunk, 0:3], b[s:s + chunk, 4:7], v0, e1, e2)
    return out


def meets64(boxes, tris, chunk=256):
    """the float64 twin: the same operations on the float32 boxes and the float32 VERTICES in double (its edges are exact differences)"""
    b = np.ascontiguousarray(boxes, f32).reshape(-1, 8).astype(np.float64)
    v0, e1, e2 = records_of(np.ascontiguousarray(tris, f32).astype(np.float64), np.float64)
    out = np.zeros((len(b), len(v0)), bool)
    for s in range(0, len(b), chunk):
        out[s:s + chunk] = meets(b[s:s + chunk, 0:3], b[s:s + chunk, 4:7], v0, e1, e2)
    return out


def degenerate(boxes):
    """boxes that are not traversed: a non-finite coordinate, lo > hi on some axis"""
    b = np.asarray(boxes, f32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(b[:, 0:3]).all(1) & np.isfinite(b[:, 4:7]).all(1) & (b[:, 0:3] <= b[:, 4:7]).all(1))


class Table:
    """Every pair's answer for (N, 8) boxes over (T, 3, 3) triangles in global id order.  mask: per-triangle bool, False = filtered out."""

    def __init__(self, boxes, tris, mask=None):
        self.b = np.ascontiguousarray(boxes, f32).reshape(-1, 8)
        self.n, self.t = len(self.b), len(tris)
        self.bad = degenerate(self.b)
        self.meets = meets32(self.b, tris) & ~self.bad[:, None]
        self.mask = np.ones(self.t, bool) if mask is None else np.asarray(mask, bool)

    def with_mask(self, mask):
        o = copy.copy(self)
        o.mask = np.ones(self.t, bool) if mask is None else np.asarray(mask, bool)
        return o

    def first(self, n):
        o = copy.copy(self)
        o.n, o.b, o.bad, o.meets = n, self.b[:n], self.bad[:n], self.meets[:n]
        return o

    def candidates(self, i, cursor=None):
        """ids of box i's candidates above the cursor g_c, ascending"""
        ids = np.nonzero(self.meets[i] & self.mask)[0]
        return ids if cursor is None else ids[ids > int(cursor)]

    def counts(self, cursors=None):
        return np.array([len(self.candidates(i, None if cursors is None else cursors[i])) for i in range(self.n)], np.uint32)

    def page(self, k, cursors=None):
        """the expected (N, k) uint32 page and the (N,) counts; cursors: None or one g_c per box"""
        out = np.full((self.n, k), MISS, np.uint32)
        cnt = np.zeros(self.n, np.uint32)
        for i in range(self.n):
            ids = self.candidates(i, None if cursors is None else cursors[i])
            cnt[i] = len(ids)
            out[i, :min(k, len(ids))] = ids[:k]
        return out, cnt


def ids_of(page):
    """a page as the uint32 words the call wrote (Renderer.overlap_boxes hands them out as int32, -1 = empty)"""
    return np.ascontiguousarray(page).view(np.uint32) if np.asarray(page).dtype != np.uint32 else np.asarray(page)


def cursors_of(page):
    """slot k - 1 of every box's page as the call reads it"""
    return ids_of(page)[:, -1].astype(np.int64).tolist()


def all_miss(page):
    return bool((ids_of(page) == MISS).all())


def pages(table, k, limit=1000):
    """the expected pages of repeated calls, the first without a cursor, until one is empty (that one included), and their counts"""
    out = []
    page, cnt = table.page(k)
    out.append((page, cnt))
    while not all_miss(page):
        assert len(out) < limit
        page, cnt = table.page(k, cursors_of(page))
        out.append((page, cnt))
    return out


def assert_pages(got, want, what=""):
    """bit for bit on every id of every page"""
    g, w = ids_of(got), ids_of(want)
    assert g.shape == w.shape, "%s: shape %s, want %s" % (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, "%s: %d of %d ids differ, first at box %d slot %d: got %s want %s" % (
        what, len(bad), g.size, bad[0][0], bad[0][1], g[bad[0][0]].tolist(), w[bad[0][0]].tolist())


def assert_counts(got, want, what=""):
    g, w = np.asarray(got).astype(np.int64).reshape(-1), np.asarray(want).astype(np.int64).reshape(-1)
    bad = np.nonzero(g != w)[0] if g.shape == w.shape else [0]
    assert g.shape == w.shape and len(bad) == 0, "%s: %d of %d counts differ, first at box %d: got %d want %d" % (
        what, len(bad), len(w), bad[0], g[bad[0]], w[bad[0]])


# ---- the walk's prune ----
def scene_slack(tris):
    """the slack as the entry point computes it: 2^-18 x max(scene extent, largest |coordinate|), rounded to float32"""
    lo, hi = tris.reshape(-1, 3).min(0).astype(np.float64), tris.reshape(-1, 3).max(0).astype(np.float64)
    return f32(max((hi - lo).max(), np.abs(lo).max(), np.abs(hi).max()) / 262144.0)


def node_skipped(blo, bhi, lo, hi, slack):
    """the kernel's node test in float32: boxes [blo, bhi] (..., 3) against the query box grown by slack; True = skipped"""
    with np.errstate(all="ignore"):
        glo, ghi = (np.asarray(lo, f32) - f32(slack)).astype(f32), (np.asarray(hi, f32) + f32(slack)).astype(f32)
        return ((bhi < glo) | (blo > ghi)).any(-1)


LEAF_SHIFT, LEAF_MASK = 27, (1 << 27) - 1


def box_walk(nodes, order, tris, box, slack):
    """k_overlap_boxes' walk of one box (8 words) over the host builder's tree (nodes (M, 16) float32: child 0's lo and hi, child 1's,
    two words, the children; order: leaf slot -> triangle): both children kept -> child 0 is entered and child 1 pushed.  Returns (the
    stack's high-water mark, the (triangle, stack slot its leaf was popped from or -1) pairs of the leaves reached, in that order)."""
    kid = np.ascontiguousarray(nodes[:, 14:16]).view(np.int32)
    lo, hi = np.asarray(box, f32)[0:3], np.asarray(box, f32)[4:7]
    stack, high, reached = [], 0, []
    node, slot = 0, -1
    while True:
        if node >= 0:
            q = nodes[node]
            k0 = not node_skipped(q[0:3], q[3:6], lo, hi, slack)
            k1 = not node_skipped(q[6:9], q[9:12], lo, hi, slack)
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
            reached += [(int(order[l]), slot) for l in range(first, first + (code >> LEAF_SHIFT) + 1)]
        if not stack:
            break
        node, slot = stack.pop(), len(stack)
    return high, reached


# ---- the cases of the GPU tests; tests/test_overlap_boxes.py asserts without a GPU that each reaches what it is named after ----
def fill_scale(k):
    """the half-extent scale of the soup boxes for pages of k: larger boxes for the larger pages"""
    return 0.08 if k <= 8 else 0.14


@functools.lru_cache(maxsize=None)
def soup_scene():
    """5 000 small triangles (above the AUTO builder's threshold of 4 096), 512 box centres in and just around their box, and per box a
    size in [0, 1) and a shape in [0.5, 1]^3"""
    rng = np.random.default_rng(7)
    tris = soup(rng, 5000, edge=0.05)
    centres = around(rng, tris, 512, 0.05)
    return tris, centres, rng.random(512), 0.5 + 0.5 * rng.random((512, 3))


def boxes_around(centres, half):
    c, half = np.asarray(centres, np.float64), np.asarray(half, np.float64)
    return boxes_of((c - half).astype(f32), (c + half).astype(f32))


@functools.lru_cache(maxsize=None)
def soup_table(scale):
    """the soup with half-extents unit x shape x scale: from no candidate to far more than a page of them"""
    tris, centres, unit, shape = soup_scene()
    return Table(boxes_around(centres, unit[:, None] * shape * scale), tris)


def fill_classes(counts, k):
    """boxes with 0, 1..k, k+1..3k and more candidates"""
    c = np.asarray(counts).astype(np.int64)
    return [int((c == 0).sum()), int(((c >= 1) & (c <= k)).sum()), int(((c > k) & (c <= 3 * k)).sum()), int((c > 3 * k).sum())]


def touching_case(twice=False):
    """Eight stacked unit quads (z = 0, 0.25, ...; triangle 2 i covers y <= x of quad i, 2 i + 1 covers y >= x) and boxes that only touch
    them, each followed by the same box one ulp back, with the ids each meets -- worked out by hand, not by the predicate.  The coordinates
    are dyadic, so that the centred frame is exact and touching in the reals is touching in float32.  twice: every triangle uploaded a
    second time (id + 16)."""
    _, tris = stacked_quads(8, 0.25)
    up, down = lambda x: np.nextafter(f32(x), f32(np.inf)), lambda x: np.nextafter(f32(x), f32(-np.inf))
    cases = [
        ("a face in the plane of quad 2", (0.25, 0.625, 0.5), (0.375, 0.75, 0.625), [5]),
        ("... one ulp above it", (0.25, 0.625, up(0.5)), (0.375, 0.75, 0.625), []),
        ("the top face in the plane of quad 3", (0.625, 0.25, 0.625), (0.75, 0.375, 0.75), [6]),
        ("... one ulp below it", (0.625, 0.25, 0.625), (0.75, 0.375, down(0.75)), []),
        ("across the diagonal of quads 2 and 3", (0.4, 0.4, 0.5), (0.6, 0.6, 0.75), [4, 5, 6, 7]),
        ("the edge x = 1 of quad 1 only", (1.0, 0.2, 0.2), (1.5, 0.4, 0.3), [2]),
        ("... one ulp off it", (up(1.0), 0.2, 0.2), (1.5, 0.4, 0.3), []),
        ("the corner (1, 1) of quads 3 and 4 only", (1.0, 1.0, 0.75), (2.0, 2.0, 1.0), [6, 7, 8, 9]),
        ("... one ulp off in x", (up(1.0), 1.0, 0.75), (2.0, 2.0, 1.0), []),
        ("... of quad 4 alone", (1.0, 1.0, 0.875), (2.0, 2.0, 1.0), [8, 9]),
        ("a flat box in the plane of quad 2", (0.125, 0.125, 0.5), (0.875, 0.875, 0.5), [4, 5]),
        ("... one ulp above it", (0.125, 0.125, up(0.5)), (0.875, 0.875, up(0.5)), []),
        ("a point box on the vertex (1, 0) of quad 5", (1.0, 0.0, 1.25), (1.0, 0.0, 1.25), [10]),
        ("... one ulp above it", (1.0, 0.0, up(1.25)), (1.0, 0.0, up(1.25)), []),
        ("a point box in the face of quad 6, off the diagonal", (0.75, 0.25, 1.5), (0.75, 0.25, 1.5), [12]),
        ("a point box on the diagonal of quad 1", (0.5, 0.5, 0.25), (0.5, 0.5, 0.25), [2, 3]),
        ("... one ulp below it", (0.5, 0.5, down(0.25)), (0.5, 0.5, down(0.25)), []),
        ("a slab through quads 1 to 6, y > x", (0.125, 0.5, 0.25), (0.25, 0.75, 1.5), [3, 5, 7, 9, 11, 13]),
        ("everything", (-1.0, -1.0, -1.0), (2.0, 2.0, 3.0), list(range(16))),
        ("beside everything", (1.5, 1.5, 0.0), (2.0, 2.0, 2.0), []),
    ]
    if twice:
        tris = np.concatenate([tris, tris])
        cases = [(name, lo, hi, ids + [g + 16 for g in ids]) for name, lo, hi, ids in cases]
    return tris, [c[0] for c in cases], boxes_of([c[1] for c in cases], [c[2] for c in cases]), [c[3] for c in cases]


@functools.lru_cache(maxsize=None)
def far_case():
    """the same kind of soup at coordinates near 4 096: the absolute rounding of fl(v0 + e) and of the centred frame dominates"""
    rng = np.random.default_rng(11)
    tris = soup(rng, 3000, edge=0.05, offset=4096.0)
    centres = around(rng, tris, 256, 0.05)
    half = rng.random((256, 3)) * rng.random((256, 1)) * 0.12
    return tris, Table(boxes_around(centres, half), tris)


@functools.lru_cache(maxsize=None)
def needle_case():
    """needles of aspect 10^4: nearly every box meets their vertex boxes and not them"""
    rng = np.random.default_rng(12)
    tris = needles(rng, 3000, 0.2, 1e4)
    centres = around(rng, tris, 256, 0.05)
    half = rng.random((256, 3)) * rng.random((256, 1)) * 0.12
    return tris, Table(boxes_around(centres, half), tris)


def spiral_boxes(n, seed=5150):
    """The boxes of the deep-tree test on deep_tree_support.spiral(n), fixed by the seed (about 130): small boxes around the origin, which
    every triangle's vertex box contains -- they keep both children at every level --, of sizes that reach only the innermost triangles,
    half of the chain and all of it; a box around each triangle's centroid, which meets the triangles from about its size outwards only;
    boxes beside everything; the whole space; and degenerate boxes."""
    from deep_tree_support import scales, spiral
    rng = np.random.default_rng(seed + n)
    s = scales(n)
    tris = spiral(n).astype(np.float64)
    c, half = [], []
    for size in (0.01 * s[0], 0.3 * s[0], s[2], s[n // 2], s[n - 4], 3.0 * s[-1]):
        c.append(rng.uniform(-1, 1, (12, 3)) * 0.01 * s[0])
        half.append(size * (0.5 + 0.5 * rng.random((12, 3))))
    cen = tris.mean(1)
    c.append(cen)
    half.append(0.2 * s[:, None] * np.ones((n, 3)))
    c.append(cen * 3.0 + s[:, None])
    half.append(0.05 * s[:, None] * np.ones((n, 3)))
    b = boxes_around(np.concatenate(c), np.concatenate(half))
    extra = boxes_of([(-FLT_MAX,) * 3, (np.nan, 0, 0), (1, 0, 0), (0, 0, -np.inf)], [(FLT_MAX,) * 3, (1, 1, 1), (0, 1, 1), (1, 1, 1)])
    return np.concatenate([b, extra])
