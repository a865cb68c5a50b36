"""Helpers of the multi-hit instanced query tests (cap_trace_instances_multi): a brute-force hit list of tests/instance_support.py --
(t, u, v, i, g) tuples in (t, instance, triangle) order -- turned into pages, cursors and counts in plain Python, as raw uint32 words."""
import numpy as np

from instance_support import MISS, bits, f32  # noqa: F401  (re-exported for the tests)

START = (-np.inf, 0, 0)  # the cursor of a first call: below every pair


def key(h):
    """(t, i, g) of a (t, u, v, i, g) tuple"""
    return (float(h[0]), int(h[3]), int(h[4]))


def above(hits, cursor):
    """the pairs strictly above the cursor (t_c, i_c, g_c) in lexicographic order"""
    return [h for h in hits if key(h) > cursor]


def page(hits, k, tmax):
    """The first k entries of `hits` as (records (k, 4) uint32, instances (k,) uint32): miss records (tmax, 0, 0, ~0) and
    instance ~0 after the last one"""
    rec = np.zeros((k, 4), f32)
    rec[:, 0] = tmax
    rec.view(np.uint32)[:, 3] = MISS
    inst = np.full(k, MISS, np.uint32)
    for j, (t, u, v, i, g) in enumerate(hits[:k]):
        rec[j, 0:3] = (t, u, v)
        rec.view(np.uint32)[j, 3] = g
        inst[j] = i
    return rec.view(np.uint32).copy(), inst


def cursor_of(rec, inst):
    """the cursor a page's last slot holds: (t, instance, triangle)"""
    return (float(np.asarray(rec, np.uint32)[-1, 0:1].view(f32)[0]), int(inst[-1]), int(np.asarray(rec, np.uint32)[-1, 3]))


def next_page(hits, k, tmax, cursor=START):
    """(records, instances, count) of one call: the page of the pairs above the cursor and their number, not capped at k"""
    rest = above(hits, cursor)
    rec, inst = page(rest, k, tmax)
    return rec, inst, len(rest)


def walk(hits, k, tmax, limit=10000):
    """Every call of a paging loop until a page comes back empty: [(records, instances, count), ...]; the last one is all miss
    records with count 0"""
    out, cursor = [], START
    while len(out) < limit:
        rec, inst, count = next_page(hits, k, tmax, cursor)
        out.append((rec, inst, count))
        if inst[0] == MISS:
            return out
        cursor = cursor_of(rec, inst)
    raise AssertionError("the walk does not end")


def listed(rec, inst):
    """the (t bits, u bits, v bits, i, g) of a page's hit slots, in order"""
    return [(int(r[0]), int(r[1]), int(r[2]), int(i), int(r[3])) for r, i in zip(np.asarray(rec, np.uint32), inst) if i != MISS or r[3] != MISS]


def words(hits):
    """a hit list as the tuples `listed` returns"""
    return [(int(bits(f32(t))[0]), int(bits(f32(u))[0]), int(bits(f32(v))[0]), int(i), int(g)) for t, u, v, i, g in hits]


def expected_pages(lists, rays, k, start=0):
    """One call over all rays, `start` pairs of each ray already paged through (a hit list is strictly ascending, so the pairs above
    the cursor the previous page left are the list from there on): (records (N, k, 4) uint32, instances (N, k) uint32, counts (N,)
    uint32)"""
    n = len(lists)
    rec, inst, cnt = np.zeros((n, k, 4), np.uint32), np.zeros((n, k), np.uint32), np.zeros(n, np.uint32)
    for j, h in enumerate(lists):
        rest = h[start:]
        rec[j], inst[j] = page(rest, k, rays[j][7])
        cnt[j] = len(rest)
    return rec, inst, cnt
