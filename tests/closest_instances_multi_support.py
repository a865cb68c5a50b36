"""Helpers of the k-nearest / in-radius closest-point tests over instances (cap_closest_instances_multi): the float32 brute force over
every (instance, triangle) pair, built on closest_instances_support.world_records and closest_point_support.cascade.  Only dist2 is
kept for all pairs -- the (N, I * T) table, whose flat index i * T + g orders ties by (i, g); the other words of a record are evaluated
again for the listed pairs alone (the same numpy operations on the same words: the same bits), so 32 instances x 600 triangles x 512
points stay in tens of MB.  candidates() is a stable sort on dist2 under radius, pair_valid and cursor; page() gives the expected record
pages, instance pages and counts, and pages() applies the cursor rule until a page is all misses."""
import copy

import numpy as np

from closest_instances_support import affine, identity, world_records
from closest_point_support import MISS, bits, cascade, degenerate, queries
from multi_hit_support import stacked_quads


class PairTable:
    """dist2 (N, I * T) float32 of (N, 4) queries against (T, 3, 3) triangles under (I, 3, 4) transforms; valid: (I, T) bool from
    closest_instances_support.pair_valid, None = every pair."""

    def __init__(self, points, M, tris, valid=None, chunk=32):
        q = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        M = np.asarray(M, np.float32).reshape(-1, 3, 4)
        tris = np.ascontiguousarray(tris, np.float32)
        self.q, self.n, self.i, self.t = q, len(q), len(M), len(tris)
        self.world = tuple(x.reshape(self.i * self.t, 3) for x in world_records(M, tris))
        self.d2 = np.zeros((self.n, self.i * self.t), np.float32)
        for s in range(0, self.n, chunk):
            e = min(self.n, s + chunk)
            self.d2[s:e] = cascade(q[s:e, 0:3], *self.world)[0]
        self.r2 = q[:, 3] * q[:, 3]
        assert self.r2.dtype == np.float32
        self.bad = degenerate(q)
        self.inst_of, self.tri_of = np.divmod(np.arange(self.i * self.t, dtype=np.int64), self.t)
        self.valid = np.ones(self.i * self.t, bool) if valid is None else np.asarray(valid, bool).reshape(-1)

    def with_radius(self, radius):
        """the same table under other radii (dist2 does not depend on them)"""
        o = copy.copy(self)
        o.q = self.q.copy()
        o.q[:, 3] = radius
        o.r2 = o.q[:, 3] * o.q[:, 3]
        o.bad = degenerate(o.q)
        return o

    def with_valid(self, valid):
        o = copy.copy(self)
        o.valid = np.ones(self.i * self.t, bool) if valid is None else np.asarray(valid, bool).reshape(-1)
        return o

    def first(self, n):
        o = copy.copy(self)
        o.n, o.q, o.r2, o.bad, o.d2 = n, self.q[:n], self.r2[:n], self.bad[:n], self.d2[:n]
        return o

    def candidates(self, i, cursor=None):
        """flat ids (inst * T + tri) of point i's candidate pairs above the cursor (dist2_c, i_c, g_c), in (dist2, inst, tri) order"""
        if self.bad[i]:
            return np.zeros(0, np.int64)
        d = self.d2[i]
        with np.errstate(invalid="ignore"):
            ok = self.valid & (d <= self.r2[i])  # (a NaN fails)
            if cursor is not None:
                dc, ic, gc = np.float32(cursor[0]), int(cursor[1]) & 0xFFFFFFFF, int(cursor[2]) & 0xFFFFFFFF
                ok &= (d > dc) | ((d == dc) & ((self.inst_of > ic) | ((self.inst_of == ic) & (self.tri_of > gc))))
        ids = np.nonzero(ok)[0]
        return ids[np.argsort(d[ids], kind="stable")]

    def records(self, i, ids):
        """the (len(ids), 8) records of point i's pairs `ids`, evaluated again"""
        out = np.zeros((len(ids), 8), np.float32)
        if len(ids) == 0:
            return out
        d2, u, v, f, pt = cascade(self.q[i:i + 1, 0:3], *(w[ids] for w in self.world))
        assert np.array_equal(bits(d2[0]), bits(self.d2[i, ids])), "the same operations give the same bits"
        out[:, 0:3], out[:, 3], out[:, 4], out[:, 5] = pt[0], d2[0], u[0], v[0]
        ob = out.view(np.uint32)
        ob[:, 6], ob[:, 7] = self.tri_of[ids], f[0]
        return out

    def miss(self, i):
        rec = np.zeros(8, np.float32)
        rec[3] = 0.0 if self.bad[i] else self.r2[i]
        rec.view(np.uint32)[6] = MISS
        return rec

    def counts(self, cursors=None):
        return np.array([len(self.candidates(i, None if cursors is None else cursors[i])) for i in range(self.n)], np.uint32)

    def page(self, k, cursors=None):
        """the expected (N, k, 8) record page, (N, k) int32 instance page (-1 in miss slots) and (N,) counts; cursors: None or one
        (dist2_c, i_c, g_c) per point"""
        out = np.zeros((self.n, k, 8), np.float32)
        inst = np.full((self.n, k), -1, np.int32)
        cnt = np.zeros(self.n, np.uint32)
        for i in range(self.n):
            ids = self.candidates(i, None if cursors is None else cursors[i])
            cnt[i] = len(ids)
            m = min(k, len(ids))
            out[i, :m] = self.records(i, ids[:m])
            inst[i, :m] = self.inst_of[ids[:m]]
            out[i, m:] = self.miss(i)
        return out, inst, cnt


def cursors_of(page, ipage):
    """slot k - 1 of every point's two pages as the call reads it: words 3 and 6 of the record, and the instance"""
    last = np.ascontiguousarray(page[:, -1, :], np.float32)
    inst = np.ascontiguousarray(ipage)[:, -1].astype(np.int64) & 0xFFFFFFFF
    return list(zip(last[:, 3].tolist(), inst.tolist(), bits(last)[:, 6].tolist()))


def all_miss(page):
    return bool((bits(page)[..., 6] == MISS).all())


def pages(table, k, limit=1000):
    """the expected (records, instances, counts) of repeated calls, the first without a cursor, until one is all misses (included)"""
    out = [table.page(k)]
    while not all_miss(out[-1][0]):
        assert len(out) < limit
        out.append(table.page(k, cursors_of(out[-1][0], out[-1][1])))
    return out


def listed(walk, i):
    """point i's (records, instances) over a list of pages, misses dropped, in the order written"""
    rows = np.concatenate([p[0][i] for p in walk])
    inst = np.concatenate([p[1][i] for p in walk])
    hit = bits(rows)[:, 6] != MISS
    assert (inst[~hit] == -1).all() and (inst[hit] >= 0).all()
    return rows[hit], inst[hit]


def assert_pair_pages(got, want, what=""):
    """bit for bit on all eight words of every record, and every instance"""
    (g_rec, g_inst), (w_rec, w_inst) = got, want
    g, w = bits(g_rec).reshape(-1, 8), bits(w_rec).reshape(-1, 8)
    assert np.shape(g_rec) == np.shape(w_rec), "%s: shape %s, want %s" % (what, np.shape(g_rec), np.shape(w_rec))
    k = max(1, np.shape(w_rec)[1]) if np.ndim(w_rec) == 3 else 1
    gi, wi = np.asarray(g_inst).astype(np.int64).reshape(-1) & 0xFFFFFFFF, np.asarray(w_inst).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    assert gi.shape == wi.shape, "%s: instance shape %s, want %s" % (what, np.shape(g_inst), np.shape(w_inst))
    bad = np.nonzero((g != w).any(1) | (gi != wi))[0]
    assert len(bad) == 0, "%s: %d of %d slots differ, first at point %d slot %d: got %s (%s) instance %d want %s (%s) instance %d" % (
        what, len(bad), len(g), bad[0] // k, bad[0] % k, np.asarray(g_rec, np.float32).reshape(-1, 8)[bad[0]].tolist(), g[bad[0], 6:8].tolist(),
        gi[bad[0]], np.asarray(w_rec, np.float32).reshape(-1, 8)[bad[0]].tolist(), w[bad[0], 6:8].tolist(), wi[bad[0]])


def assert_counts(got, want, what=""):
    g, w = np.asarray(got).astype(np.int64).reshape(-1), np.asarray(want).astype(np.int64).reshape(-1)
    bad = np.nonzero(g != w)[0]
    assert g.shape == w.shape and len(bad) == 0, "%s: %d of %d counts differ, first at point %d: got %d want %d" % (
        what, len(bad), len(w), bad[0], g[bad[0]], w[bad[0]])


def tie_case():
    """(triangles, transforms, queries): stacked_quads under three coincident instances and one shifted by a quad spacing.  Every point
    lies over the quads' shared diagonal, so both triangles of a plane tie, in all four instances: eight pairs per plane distance.
    Even points stand a quarter of the spacing above a plane with three planes in reach (24 pairs over 3 distinct dist2), odd ones
    midway between two planes with those two in reach (16 pairs at one dist2).  All coordinates are dyadic: the ties are exact."""
    _, tris = stacked_quads(40, 0.25)
    M = np.stack([identity()[0], identity()[0], identity()[0], affine(np.eye(3), (0, 0, 0.25))])
    pts, radii = [], []
    for n, j in enumerate(range(3, 35)):
        xy = (0.5, 0.25, 0.75)[n % 3]
        pts.append((xy, xy, (j + (0.25 if n % 2 == 0 else 0.5)) * 0.25))
        radii.append(0.32 if n % 2 == 0 else 0.2)
    return tris, M, queries(pts, np.float32(radii))
