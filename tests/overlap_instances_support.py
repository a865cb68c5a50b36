"""Helpers of the instanced box overlap tests (cap_overlap_instances): the float32 brute force -- closest_instances_support.world_records
for the world record of every (instance, triangle), overlap_support.meets for the predicate on it, pair_valid for masks and objects --,
the pair table with candidates / page / counts / pages() under the (i, g) cursor, bit-for-bit asserts, a numpy model of the prune and
the debug entry's wrapper, and the case builders of the GPU tests."""
import copy
import ctypes as C
import functools

import numpy as np

from closest_instances_support import affine, identity, near_translations, pair_valid, world_records  # noqa: F401
from closest_point_support import needles, soup
from instance_support import regular_transforms
from overlap_support import FLT_MAX, MISS, boxes_of, degenerate, ids_of, meets, touching_case  # noqa: F401

f32 = np.float32
EPS32 = f32(2.0 ** -24)
C2 = f32(96.0)  # cap_near.h kOverlapC2


def meets_pairs(boxes, M, tris, dtype=np.float32, chunk=32):
    """(N, I * T) bool: the contract's predicate on the world record of every pair, flat index i * T + g.  dtype=float64 is the twin:
    the same operations on the float32 boxes, transforms and vertices in double."""
    b = np.ascontiguousarray(boxes, f32).reshape(-1, 8).astype(dtype)
    M = np.asarray(M, f32).reshape(-1, 3, 4)
    v0w, e1w, e2w = (x.reshape(-1, 3) for x in world_records(M, np.ascontiguousarray(tris, f32), dtype))
    out = np.zeros((len(b), len(v0w)), bool)
    for s in range(0, len(b), chunk):
        out[s:s + chunk] = meets(b[s:s + chunk, 0:3], b[s:s + chunk, 4:7], v0w, e1w, e2w)
    return out


class PairTable:
    """Every pair's answer for (N, 8) world boxes over (T, 3, 3) triangles under (I, 3, 4) transforms.  valid: (I, T) bool from
    closest_instances_support.pair_valid, None = every pair."""

    def __init__(self, boxes, M, tris, valid=None):
        self.b = np.ascontiguousarray(boxes, f32).reshape(-1, 8)
        M = np.asarray(M, f32).reshape(-1, 3, 4)
        self.n, self.i, self.t = len(self.b), len(M), len(tris)
        self.bad = degenerate(self.b)
        self.meets = meets_pairs(self.b, M, tris) & ~self.bad[:, None]
        self.inst_of, self.tri_of = np.divmod(np.arange(self.i * self.t, dtype=np.int64), self.t)
        self.valid = np.ones(self.i * self.t, bool) if valid is None else np.asarray(valid, bool).reshape(-1)

    def with_valid(self, valid):
        o = copy.copy(self)
        o.valid = np.ones(self.i * self.t, bool) if valid is None else np.asarray(valid, bool).reshape(-1)
        return o

    def first(self, n):
        o = copy.copy(self)
        o.n, o.b, o.bad, o.meets = n, self.b[:n], self.bad[:n], self.meets[:n]
        return o

    def candidates(self, b, cursor=None):
        """flat ids (i * T + g) of box b's pairs lexicographically above the cursor (i_c, g_c), in (i, g) order"""
        ok = self.meets[b] & self.valid
        if cursor is not None:
            ic, gc = int(cursor[0]) & 0xFFFFFFFF, int(cursor[1]) & 0xFFFFFFFF
            ok = ok & ((self.inst_of > ic) | ((self.inst_of == ic) & (self.tri_of > gc)))
        return np.nonzero(ok)[0]

    def counts(self, cursors=None):
        return np.array([len(self.candidates(b, None if cursors is None else cursors[b])) for b in range(self.n)], np.uint32)

    def page(self, k, cursors=None):
        """the expected (N, k) uint32 triangle page, (N, k) uint32 instance page and (N,) counts; cursors: None or one (i_c, g_c) per box"""
        tri = np.full((self.n, k), MISS, np.uint32)
        inst = np.full((self.n, k), MISS, np.uint32)
        cnt = np.zeros(self.n, np.uint32)
        for b in range(self.n):
            ids = self.candidates(b, None if cursors is None else cursors[b])
            cnt[b] = len(ids)
            m = min(k, len(ids))
            tri[b, :m], inst[b, :m] = self.tri_of[ids[:m]], self.inst_of[ids[:m]]
        return tri, inst, cnt


def cursors_of(tri, inst):
    """slot k - 1 of every box's two pages as the call reads it: (i_c, g_c)"""
    return list(zip(ids_of(inst)[:, -1].astype(np.int64).tolist(), ids_of(tri)[:, -1].astype(np.int64).tolist()))


def all_miss(tri):
    return bool((ids_of(tri) == MISS).all())


def pages(table, k, limit=1000):
    """the expected (triangles, instances, counts) of repeated calls, the first without a cursor, until one is empty (included)"""
    out = [table.page(k)]
    while not all_miss(out[-1][0]):
        assert len(out) < limit
        out.append(table.page(k, cursors_of(out[-1][0], out[-1][1])))
    return out


def assert_pair_pages(got, want, what=""):
    """bit for bit on every triangle and every instance of every page"""
    (g_tri, g_inst), (w_tri, w_inst) = got, want
    gt, gi, wt, wi = ids_of(g_tri), ids_of(g_inst), ids_of(w_tri), ids_of(w_inst)
    assert gt.shape == wt.shape and gi.shape == wi.shape, "%s: shapes %s %s, want %s %s" % (what, gt.shape, gi.shape, wt.shape, wi.shape)
    bad = np.argwhere((gt != wt) | (gi != wi))
    assert len(bad) == 0, "%s: %d of %d slots differ, first at box %d slot %d: got triangles %s instances %s want %s %s" % (
        what, len(bad), gt.size, bad[0][0], bad[0][1], gt[bad[0][0]].tolist(), gi[bad[0][0]].tolist(), wt[bad[0][0]].tolist(), wi[bad[0][0]].tolist())


def assert_counts(got, want, what=""):
    g, w = np.asarray(got).astype(np.int64).reshape(-1), np.asarray(want).astype(np.int64).reshape(-1)
    bad = np.nonzero(g != w)[0] if g.shape == w.shape else [0]
    assert g.shape == w.shape and len(bad) == 0, "%s: %d of %d counts differ, first at box %d: got %d want %d" % (
        what, len(bad), len(w), bad[0], g[bad[0]], w[bad[0]])


def fill_classes(counts, k):
    """boxes with 0, 1..k, k+1..3k and more pairs"""
    c = np.asarray(counts).astype(np.int64)
    return [int((c == 0).sum()), int(((c >= 1) & (c <= k)).sum()), int(((c > k) & (c <= 3 * k)).sum()), int((c > 3 * k).sum())]


# ---- the prune: the debug entry, and the same arithmetic in numpy with the constant as a parameter ----
def prune(M, object_lo, object_hi, world_lo, world_hi, node_lo, node_hi, box_lo, box_hi, lib=None):
    """cap_debug_overlap_instance_prune: {W, g, xw, slack, image_lo, image_hi, skip_top, skip_node}"""
    if lib is None:
        from capsaicin_amd import capi
        lib = capi.lib()
    f3 = C.c_float * 3
    v = lambda x: f3(*np.asarray(x, f32).reshape(3).tolist())
    m = (C.c_float * 12)(*np.asarray(M, f32).reshape(12).tolist())
    W, ilo, ihi = (C.c_float * 12)(), f3(), f3()
    g, xw, slack, top, node = C.c_float(), C.c_float(), C.c_float(), C.c_uint32(), C.c_uint32()
    rc = lib.cap_debug_overlap_instance_prune(m, v(object_lo), v(object_hi), v(world_lo), v(world_hi), v(node_lo), v(node_hi), v(box_lo), v(box_hi), W,
                                              C.byref(g), C.byref(xw), C.byref(slack), ilo, ihi, C.byref(top), C.byref(node))
    assert rc == 0, lib.cap_last_error()
    return dict(W=np.array(W[:], f32).reshape(3, 4), g=g.value, xw=xw.value, slack=slack.value, image_lo=np.array(ilo[:], f32),
                image_hi=np.array(ihi[:], f32), skip_top=int(top.value), skip_node=int(node.value))


def model_image(W, g, xw, box_lo, box_hi, c2=C2):
    """cap_near.h overlap_slack and overlap_image in float32 numpy, one rounded operation per operation there: (slack, image lo, image hi)
    of boxes (..., 3) under the stored W (3, 4)"""
    W, lo, hi = np.asarray(W, f32), np.asarray(box_lo, f32), np.asarray(box_hi, f32)
    with np.errstate(all="ignore"):
        hl, hh = lo * f32(0.5), hi * f32(0.5)
        c, h = hl + hh, hh - hl
        bmax = np.maximum(np.abs(lo), np.abs(hi)).max(-1)
        slack = (f32(c2) * EPS32) * (bmax + f32(xw))
        s = (slack / f32(g))[..., None]
        A = np.abs(W)
        cp = np.stack([((W[r, 0] * c[..., 0] + W[r, 1] * c[..., 1]) + W[r, 2] * c[..., 2]) + W[r, 3] for r in range(3)], -1)
        hp = np.stack([(A[r, 0] * h[..., 0] + A[r, 1] * h[..., 1]) + A[r, 2] * h[..., 2] for r in range(3)], -1)
        assert cp.dtype == f32 and hp.dtype == f32 and s.dtype == f32
        return slack, (cp - hp) - s, (cp + hp) + s


def model_miss(blo, bhi, qlo, qhi):
    """cap_near.h overlap_miss: True where the box [blo, bhi] lies beyond [qlo, qhi] on some axis (a NaN compares false)"""
    with np.errstate(invalid="ignore"):
        return ((np.asarray(bhi, f32) < qlo) | (qhi < np.asarray(blo, f32))).any(-1)


def model_skips(W, g, xw, world_lo, world_hi, node_lo, node_hi, box_lo, box_hi, c2=C2):
    """(skip at the top level, skip at the node) of the model, arrays over the leading axes"""
    slack, olo, ohi = model_image(W, g, xw, box_lo, box_hi, c2)
    with np.errstate(all="ignore"):
        glo, ghi = np.asarray(box_lo, f32) - slack[..., None], np.asarray(box_hi, f32) + slack[..., None]
    return model_miss(world_lo, world_hi, glo, ghi), model_miss(node_lo, node_hi, olo, ohi)


def stand_in_boxes(M, tris):
    """What stands for the boxes above a triangle, the tightest they can be: its own float32 vertex box in object space (T, 3) x 2, and
    per instance the box of the exact images of its vertices rounded outwards to float32 (I, T, 3) x 2 -- the stored world boxes hold
    M(object box)."""
    t = np.asarray(tris, f32)
    Md = np.asarray(M, f32).reshape(-1, 3, 4).astype(np.float64)
    with np.errstate(all="ignore"):
        w = np.einsum("irk,tvk->itvr", Md[:, :, :3], t.astype(np.float64)) + Md[:, None, None, :, 3]
        wlo, whi = np.nextafter(w.min(2).astype(f32), f32(-np.inf)), np.nextafter(w.max(2).astype(f32), f32(np.inf))
    return t.min(1), t.max(1), wlo, whi


# ---- the cases of the GPU tests; tests/test_overlap_instances.py asserts without a GPU that each reaches what it is named after ----
def boxes_near(rng, M, tris, n, size=0.3, away=8):
    """n world boxes centred near random world points of random triangles of random instances, half-extents rng x rng x size x the
    instance's scale ||L||_F / sqrt 3 per axis; every `away`-th box is moved off by three scales (most of those meet nothing)"""
    Md = np.asarray(M, f32).astype(np.float64)
    i, g = rng.integers(0, len(Md), n), rng.integers(0, len(tris), n)
    x = np.einsum("nk,nkj->nj", rng.dirichlet((1, 1, 1), n), np.asarray(tris, np.float64)[g])
    y = np.einsum("nrk,nk->nr", Md[i][:, :, :3], x) + Md[i][:, :, 3]
    scale = np.linalg.norm(Md[i][:, :, :3], axis=(1, 2)) / np.sqrt(3.0)
    half = rng.random((n, 3)) * rng.random((n, 1)) * size * scale[:, None]
    c = y + (rng.random((n, 3)) - 0.5) * half
    c[::away] += 3.0 * scale[::away, None]
    return boxes_of((c - half).astype(f32), (c + half).astype(f32))


@functools.lru_cache(maxsize=None)
def soup_case():
    """600 small triangles under 32 regular transforms, four of them copies of another one (two exact, two moved by a hundredth of
    their size) so that pages span instances; 512 boxes: (triangles, transforms, table)"""
    tris = soup(np.random.default_rng(3), 600, edge=0.05)
    M = regular_transforms(32).copy()
    for j in (5, 12, 20, 27):
        M[j] = M[j - 4]
    for j in (20, 27):
        M[j, :, 3] += f32(0.01) * np.abs(M[j, :, :3]).max()
    return tris, M, PairTable(boxes_near(np.random.default_rng(31), M, tris, 512), M, tris)


@functools.lru_cache(maxsize=None)
def far_case():
    """the same soup with the translations near 4 096: the world record's rounding of 2^-12 against triangles of size 0.05"""
    tris = soup(np.random.default_rng(3), 600, edge=0.05)
    M = near_translations(regular_transforms(32))
    return tris, M, PairTable(boxes_near(np.random.default_rng(32), M, tris, 256), M, tris)


@functools.lru_cache(maxsize=None)
def needle_case():
    """needles of aspect 10^4 under 16 transforms: nearly every box meets their vertex boxes and not them"""
    tris = needles(np.random.default_rng(12), 600, 0.2, 1e4)
    M = regular_transforms(16)
    return tris, M, PairTable(boxes_near(np.random.default_rng(33), M, tris, 256), M, tris)


def huge_boxes():
    """FLT_MAX, lopsided huge and degenerate boxes (the first six are traversed)"""
    nan, inf = f32(np.nan), f32(np.inf)
    lo = [(-FLT_MAX,) * 3, (-FLT_MAX, -FLT_MAX, -FLT_MAX), (-FLT_MAX, -1e30, -FLT_MAX), (-FLT_MAX, 0.5, -FLT_MAX), (0, 0, 0), (-1e38, -1e38, -1e38),
          (nan, 0, 0), (0, 0, 0), (0, 0, -inf), (0.75, 0, 0), (0, 0, 0), (nan,) * 3]
    hi = [(FLT_MAX,) * 3, (0, 0, 0), (FLT_MAX, FLT_MAX, 0), (FLT_MAX, 0.5, FLT_MAX), (FLT_MAX,) * 3, (1e38, 0, 1e38),
          (1, 1, 1), (1, inf, 1), (1, 1, 1), (0.25, 1, 1), (1, 1, nan), (nan,) * 3]
    return boxes_of(lo, hi)


def touching_instances():
    """touching_case()'s quads under a power-of-two translation and under diag(2, 1, 1): (triangles, transforms, names, world boxes,
    the (instance, triangle) pairs each box meets, worked out by hand: instance 0's boxes are the case's moved by the translation,
    instance 1's the case's with x doubled and moved -- both maps are exact on the dyadic coordinates, and the images lie far enough
    apart not to meet each other.  A coordinate the case moved one ulp off a dyadic value is one ulp of its IMAGE off again."""
    tris, names, boxes, want = touching_case()
    t = np.array([64.0, -32.0, 16.0])
    M = np.stack([affine(np.eye(3), t), affine(np.diag([2.0, 1.0, 1.0]), (-64.0, 0.0, 0.0))])

    def image(scale, move):
        x = boxes[:, [0, 1, 2, 4, 5, 6]].astype(np.float64) * np.tile(scale, 2) + np.tile(move, 2)  # (exact in double)
        r = x.astype(f32)
        r = np.where(x > r, np.nextafter(r, f32(np.inf)), np.where(x < r, np.nextafter(r, f32(-np.inf)), r))
        return boxes_of(r[:, 0:3], r[:, 3:6])

    b0, b1 = image(np.ones(3), t), image(np.array([2.0, 1.0, 1.0]), np.array([-64.0, 0.0, 0.0]))
    pairs = [[(0, g) for g in ids] for ids in want] + [[(1, g) for g in ids] for ids in want]
    return tris, M, ["translated: " + n for n in names] + ["stretched: " + n for n in names], np.concatenate([b0, b1]), pairs
