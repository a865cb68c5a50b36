"""Helpers of the k-nearest / in-radius closest-point tests (cap_closest_points_multi): the float32 brute force over every triangle, built
on closest_point_support's transcription of the contract -- the (N, T) dist2 table with the other words of every pair's record, a point's
candidates under radius, mask and cursor in (dist2, id) order, the expected (N, k, 8) pages and counts, and pages(), which applies the
cursor rule until nothing is left."""
import copy

import numpy as np

from closest_point_support import MISS, bits, cascade, degenerate, records_of


class Table:
    """Every pair's record for (N, 4) queries over (T, 3, 3) triangles in global id order: dist2, u, v (N, T) float32, feature (N, T)
    uint32, point (N, T, 3) float32; r2 = fl(radius * radius) and the degenerate queries.  mask: per-triangle bool, False = filtered out."""

    def __init__(self, points, tris, mask=None, chunk=128):
        q = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        v0, e1, e2 = records_of(np.ascontiguousarray(tris, np.float32))
        n, t = len(q), len(v0)
        self.q, self.n, self.t = q, n, t
        self.d2, self.u, self.v = (np.zeros((n, t), np.float32) for _ in range(3))
        self.f, self.pt = np.zeros((n, t), np.uint32), np.zeros((n, t, 3), np.float32)
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            self.d2[s:e], self.u[s:e], self.v[s:e], self.f[s:e], self.pt[s:e] = cascade(q[s:e, 0:3], v0, e1, e2)
        self.r2 = q[:, 3] * q[:, 3]
        assert self.r2.dtype == np.float32
        self.bad = degenerate(q)
        self.mask = np.ones(t, bool) if mask is None else np.asarray(mask, bool)

    def with_radius(self, radius):
        """the same table under other radii (the per-pair records do not depend on them)"""
        o = copy.copy(self)
        o.q = self.q.copy()
        o.q[:, 3] = radius
        o.r2 = o.q[:, 3] * o.q[:, 3]
        o.bad = degenerate(o.q)
        return o

    def first(self, n):
        """the table of the first n queries"""
        o = copy.copy(self)
        o.n, o.q, o.r2, o.bad = n, self.q[:n], self.r2[:n], self.bad[:n]
        o.d2, o.u, o.v, o.f, o.pt = self.d2[:n], self.u[:n], self.v[:n], self.f[:n], self.pt[:n]
        return o

    def with_mask(self, mask):
        o = copy.copy(self)
        o.mask = np.ones(self.t, bool) if mask is None else np.asarray(mask, bool)
        return o

    def candidates(self, i, cursor=None):
        """ids of point i's candidates above the cursor (dist2_c, g_c), in (dist2, id) order: stable sort of the ids by dist2"""
        if self.bad[i]:
            return np.zeros(0, np.int64)
        d = self.d2[i]
        with np.errstate(invalid="ignore"):
            ok = self.mask & (d <= self.r2[i])  # (a NaN fails)
            if cursor is not None:
                dc, gc = np.float32(cursor[0]), int(cursor[1])
                ok &= (d > dc) | ((d == dc) & (np.arange(self.t) > gc))
        ids = np.nonzero(ok)[0]
        return ids[np.argsort(d[ids], kind="stable")]

    def record(self, i, g):
        rec = np.zeros(8, np.float32)
        rec[0:3], rec[3], rec[4], rec[5] = self.pt[i, g], self.d2[i, g], self.u[i, g], self.v[i, g]
        rec.view(np.uint32)[6:8] = (g, self.f[i, g])
        return rec

    def miss(self, i):
        rec = np.zeros(8, np.float32)
        rec[3] = 0.0 if self.bad[i] else self.r2[i]
        rec.view(np.uint32)[6] = MISS
        return rec

    def counts(self, cursors=None):
        return np.array([len(self.candidates(i, None if cursors is None else cursors[i])) for i in range(self.n)], np.uint32)

    def page(self, k, cursors=None):
        """the expected (N, k, 8) page and the (N,) counts; cursors: None or one (dist2_c, g_c) per point"""
        out = np.zeros((self.n, k, 8), np.float32)
        cnt = np.zeros(self.n, np.uint32)
        for i in range(self.n):
            ids = self.candidates(i, None if cursors is None else cursors[i])
            cnt[i] = len(ids)
            for j in range(k):
                out[i, j] = self.record(i, ids[j]) if j < len(ids) else self.miss(i)
        return out, cnt


def cursors_of(page):
    """slot k - 1 of every point's page as the call reads it: words 3 and 6"""
    last = np.ascontiguousarray(page[:, -1, :], np.float32)
    return list(zip(last[:, 3].tolist(), bits(last)[:, 6].tolist()))


def all_miss(page):
    return bool((bits(page)[..., 6] == MISS).all())


def pages(table, k, limit=1000):
    """the expected pages of repeated calls, the first without a cursor, until one is all misses (that one included), and their counts"""
    out = []
    page, cnt = table.page(k)
    out.append((page, cnt))
    while not all_miss(page):
        assert len(out) < limit
        page, cnt = table.page(k, cursors_of(page))
        out.append((page, cnt))
    return out


def listed(page_list, i):
    """point i's records over a list of pages, misses dropped, in the order written"""
    rows = np.concatenate([p[i] for p in page_list])
    return rows[bits(rows)[:, 6] != MISS]


def assert_pages(got, want, what=""):
    """bit for bit on all eight words of every record"""
    g, w = bits(got).reshape(-1, 8), bits(want).reshape(-1, 8)
    assert g.shape == w.shape, "%s: shape %s, want %s" % (what, np.shape(got), np.shape(want))
    bad = np.nonzero((g != w).any(1))[0]
    k = max(1, np.shape(want)[1]) if np.ndim(want) == 3 else 1
    assert len(bad) == 0, "%s: %d of %d records differ, first at point %d slot %d: got %s (%s) want %s (%s)" % (
        what, len(bad), len(g), bad[0] // k, bad[0] % k, np.asarray(got, np.float32).reshape(-1, 8)[bad[0]].tolist(), g[bad[0], 6:8].tolist(),
        np.asarray(want, np.float32).reshape(-1, 8)[bad[0]].tolist(), w[bad[0], 6:8].tolist())


def assert_counts(got, want, what=""):
    g, w = np.asarray(got).astype(np.int64).reshape(-1), np.asarray(want).astype(np.int64).reshape(-1)
    bad = np.nonzero(g != w)[0]
    assert g.shape == w.shape and len(bad) == 0, "%s: %d of %d counts differ, first at point %d: got %d want %d" % (
        what, len(bad), len(w), bad[0], g[bad[0]], w[bad[0]])
