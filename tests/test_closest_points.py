"""Closest-point queries (cap_closest_points) without a GPU: the header's prototype, the export and the binding; the numpy transcription
of the contract (closest_point_support.py) pinned by hand and judged against its float64 twin; and the address checks of the call's
two arrays."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import EPS, MISS, argmin_lex, bits, cascade, closest, queries, records_of, soup
from multi_hit_support import stacked_quads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID_ARG = 0, 1


def test_header_prototype_compiles(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "closest.c"
    src.write_text("""#include <stddef.h>
#include "capsaicin_hip.h"
_Static_assert(sizeof(CapPointDesc) == 16 && offsetof(CapPointDesc, radius) == 12, "CapPointDesc");
_Static_assert(sizeof(CapClosest) == 32 && offsetof(CapClosest, dist2) == 12 && offsetof(CapClosest, u) == 16 && offsetof(CapClosest, triangle) == 24 &&
               offsetof(CapClosest, feature) == 28, "CapClosest");
_Static_assert(CAP_FEATURE_FACE == 0 && CAP_FEATURE_EDGE_V0V1 == 1 && CAP_FEATURE_EDGE_V1V2 == 2 && CAP_FEATURE_EDGE_V2V0 == 3 && CAP_FEATURE_V0 == 4 &&
               CAP_FEATURE_V1 == 5 && CAP_FEATURE_V2 == 6, "features");
int (*const closest)(CapContext*, const CapPointDesc*, uint64_t, CapClosest*, const CapTraceOptions*) = cap_closest_points;
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "closest.o")])


def test_entry_point_is_exported_and_bound(native_lib):
    assert hasattr(native_lib, "cap_closest_points")
    assert len(capi.SYMBOLS["cap_closest_points"][1]) == 5
    assert C.sizeof(capi.PointDesc) == 16 and C.sizeof(capi.Closest) == 32
    assert capi.Closest.dist2.offset == 12 and capi.Closest.triangle.offset == 24 and capi.Closest.feature.offset == 28
    assert callable(capi.Renderer.closest_points)
    assert native_lib.cap_closest_points(None, None, 0, None, None) == ERR_INVALID_ARG
    assert b"cap_closest_points: ctx is NULL" in native_lib.cap_last_error()


def test_closest_triangles_reads_id_and_feature():
    rec = np.zeros((3, 8), np.float32)
    rec.view(np.uint32)[:, 6] = (7, MISS, 1 << 31)
    rec.view(np.uint32)[:, 7] = (6, 0, 3)
    ids, feat = capi.closest_triangles(rec)
    assert ids.tolist() == [7, MISS, 1 << 31] and feat.tolist() == [6, 0, 3]
    import torch
    ids_t, feat_t = capi.closest_triangles(torch.from_numpy(rec))
    assert ids_t.tolist() == [7, MISS, 1 << 31] and feat_t.tolist() == [6, 0, 3]


# ---- the reference pinned by hand ----
UNIT = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
# point, feature, (u, v), closest point, dist2: every value exact in binary32
FEATURES = [((0.25, 0.25, 1.0), 0, (0.25, 0.25), (0.25, 0.25, 0), 1.0),
            ((0.5, -1.0, 0.0), 1, (0.5, 0.0), (0.5, 0, 0), 1.0),
            ((1.0, 1.0, 0.0), 2, (0.5, 0.5), (0.5, 0.5, 0), 0.5),
            ((-1.0, 0.5, 0.0), 3, (0.0, 0.5), (0, 0.5, 0), 1.0),
            ((-1.0, -1.0, 0.0), 4, (0.0, 0.0), (0, 0, 0), 2.0),
            ((2.0, -0.5, 0.0), 5, (1.0, 0.0), (1, 0, 0), 1.25),
            ((-0.5, 2.0, 0.0), 6, (0.0, 1.0), (0, 1, 0), 1.25)]


@pytest.mark.parametrize("case", FEATURES, ids=[str(c[1]) for c in FEATURES])
def test_each_feature_on_one_triangle(case):
    p, feature, uv, q, d2 = case
    rec, _ = closest(queries([p]), UNIT)
    assert rec[0, 0:3].tolist() == list(q) and rec[0, 3] == d2 and rec[0, 4:6].tolist() == list(uv)
    assert bits(rec)[0, 6:8].tolist() == [0, feature]


def test_stacked_quads_ties():
    _, tris = stacked_quads(40, 0.25)
    q = queries([(0.5, 0.5, 0.125), (2, 2, 0.125), (0.5, 0.25, 0.125)])
    rec, table = closest(q, tris)
    v0, e1, e2 = records_of(tris)
    _, _, _, feat, _ = cascade(q[:, 0:3], v0, e1, e2)
    for i, (d2, tied, features) in enumerate(((0.015625, [0, 1, 2, 3], [3, 1, 3, 1]), (2.015625, [0, 1, 2, 3], [6, 5, 6, 5]), (0.015625, [0, 2], [0, 0]))):
        assert np.nonzero(table[i] == table[i].min())[0].tolist() == tied and table[i].min() == np.float32(d2)
        assert feat[i, tied].tolist() == features
        assert rec[i, 3] == np.float32(d2) and bits(rec)[i, 6] == 0, "the lowest id of the tie"
    assert bits(rec)[:, 7].tolist() == [3, 6, 0]


def test_radius_and_miss_records():
    rec, _ = closest(np.float32([[0.25, 0.25, 1, 1.0], [0.25, 0.25, 1, 0.99999994], [0.25, 0.25, 0, 0.0], [0.25, 0.25, 1, 0.0]]), UNIT)
    assert bits(rec)[:, 6].tolist() == [0, MISS, 0, MISS], "dist2 <= r2 is inclusive; radius 0 admits dist2 == 0 only"
    miss = np.zeros(8, np.float32)
    miss[3] = np.float32(0.99999994) * np.float32(0.99999994)
    miss.view(np.uint32)[6] = MISS
    assert np.array_equal(bits(rec[1]), bits(miss)), "the miss record carries r2"
    assert rec[3, 3] == 0.0


def test_degenerate_queries_give_the_miss_record_with_dist2_zero():
    nan, inf = np.nan, np.inf
    q = np.float32([[nan, 0, 0, 1], [0, inf, 0, 1], [0, 0, -inf, inf], [0, 0, 0, -1], [0, 0, 0, nan], [0, 0, 0, -0.0]])
    rec, _ = closest(q, UNIT)
    want = np.zeros(8, np.uint32)
    want[6] = MISS
    for i in range(5):
        assert np.array_equal(bits(rec[i]), want), i
    assert bits(rec)[5, 6] == 0, "radius -0 is radius 0: the vertex itself is at dist2 0"


def test_a_triangle_whose_dist2_is_nan_is_never_the_answer():
    """v0 == v1: for a point on v2's side the cascade reaches edge v0v1 with 0 / 0.  The NaN fails `dist2 <= r2` and every comparison of
    the tie rule.  (A zero-area triangle with three distinct collinear vertices has finite weights and answers as the segment it is.)"""
    flat = np.float32([[0, 0, 0], [0, 0, 0], [0, 1, 0]])
    far = np.float32([[5, 0, 0], [6, 0, 0], [5, 1, 0]])
    q = queries([(0.1, 0.5, 0.0)])
    v0, e1, e2 = records_of(flat[None])
    assert np.isnan(cascade(q[:, 0:3], v0, e1, e2)[0][0, 0])
    rec, _ = closest(q, flat[None])
    assert bits(rec)[0, 6] == MISS and rec[0, 3] == np.inf
    for tris, winner in ((np.stack([flat, far]), 1), (np.stack([far, flat]), 0)):
        rec, _ = closest(q, tris)
        assert bits(rec)[0, 6] == winner
    segment = np.float32([[[0, 0, 0], [2, 0, 0], [1, 0, 0]]])
    rec, _ = closest(queries([(0.5, 1.0, 0.0)]), segment)
    assert bits(rec)[0, 6] == 0 and rec[0, 3] == 1.0


def test_mask_restricts_the_candidates():
    _, tris = stacked_quads(4, 0.25)
    mask = np.arange(len(tris)) >= 4
    rec, _ = closest(queries([(0.5, 0.25, 0.0)]), tris, mask)
    assert bits(rec)[0, 6] == 4 and rec[0, 3] == np.float32(0.25)
    rec, _ = closest(queries([(0.5, 0.25, 0.0)], 0.25), tris, mask)
    assert bits(rec)[0, 6] == MISS and rec[0, 3] == np.float32(0.0625)


def test_argmin_prefers_the_lower_id_and_skips_invalid_entries():
    d = np.float32([[3, 1, 1, 0.5], [np.inf, np.inf, 2, 2], [np.nan, np.inf, np.inf, np.nan]])
    valid = np.array([[1, 1, 1, 0], [0, 0, 0, 0], [0, 0, 1, 0]], bool)
    assert argmin_lex(d, valid).tolist() == [1, -1, 2]


# ---- the reference against its float64 twin ----
# The distance is sqrt(dist2).  Rounding on the float32 path, in units of eps = 2^-24 and for weights in [0, 1]: ap carries 1 |ap|; the
# two products and the sum of m = e1 u + e2 v carry 2 (|e1| + |e2|); delta = ap - m one more of each, and the dot product and the
# square root less than 3 of the distance itself, which is at most |ap| + |e1| + |e2|: 6 (|ap| + |e1| + |e2|) in all for exact weights.
# A weight is a quotient of differences of products of the d's: four to six roundings, amplified by the triangle's shape -- the soup's
# triangles are no thinner than 0.2 (shortest altitude over longest edge), which bounds that amplification by 1 / 0.2^2 = 25 -- and a
# weight's error moves the point by its edge, but the distance only to first order in the component along delta: 6 * 25 (|e1| + |e2|)
# is generous.  K = 6 + 150, rounded up to a power of two.
K_MARGIN = 256.0


def test_reference_against_float64():
    rng = np.random.default_rng(20260)
    tris = soup(rng, 4000, edge=0.05, offset=100.0)
    pts = (100.0 + rng.random((500, 3)) * 1.2 - 0.1).astype(np.float32)
    v0, e1, e2 = records_of(tris)
    w0, w1, w2 = records_of(tris, np.float64)
    d32, _, _, _, _ = cascade(pts, v0, e1, e2)
    d64, _, _, _, _ = cascade(pts.astype(np.float64), w0, w1, w2)
    assert d32.dtype == np.float32 and d64.dtype == np.float64
    ap = np.linalg.norm(pts.astype(np.float64)[:, None, :] - w0[None], axis=2)
    margin = K_MARGIN * EPS * (ap + np.linalg.norm(w1, axis=1)[None] + np.linalg.norm(w2, axis=1)[None])
    err = np.abs(np.sqrt(d32.astype(np.float64)) - np.sqrt(d64))
    print("largest distance error %.3g, in margins %.3g" % (err.max(), (err / margin).max()))
    assert np.all(err <= margin)
    g32 = argmin_lex(d32, np.ones(d32.shape, bool))
    order = np.argsort(d64, axis=1)[:, :2]
    rows = np.arange(len(pts))
    best, second = np.sqrt(d64[rows, order[:, 0]]), np.sqrt(d64[rows, order[:, 1]])
    clear = second - best > margin[rows, order[:, 0]] + margin[rows, order[:, 1]]
    assert clear.sum() > 0.9 * len(pts)
    assert np.array_equal(g32[clear], order[clear, 0])


# ---- the address checks for the call's two arrays: points (16 B, 16-aligned), records (32 B, 16-aligned) ----
LAYOUT = [(16, 16), (32, 16)]
BASE = 0x7F0000010000
TOP = 1 << 64


def range_cases():
    """(label, n, bases, expected code, substrings of the message)"""
    n, out = 5, []
    apart = [BASE, BASE + n * 16 + 64]
    out.append(("aligned and disjoint", n, apart, OK, ()))
    for i in range(2):
        for off in (4, 8, 12):
            b = list(apart)
            b[i] += off
            out.append(("range %d misaligned by %d" % (i, off), n, b, ERR_INVALID_ARG, ("range %d" % i, "16-byte aligned")))
    out.append(("records right behind the points", n + 1, [BASE, BASE + (n + 1) * 16], OK, ()))
    out.append(("points right behind the records", n + 1, [BASE + (n + 1) * 32, BASE], OK, ()))
    out.append(("records start in the last point", n, [BASE, BASE + (n - 1) * 16], ERR_INVALID_ARG, ("range 0", "range 1", "overlap")))
    out.append(("points start in the last record", n, [BASE + (n - 1) * 32, BASE], ERR_INVALID_ARG, ("range 0", "range 1", "overlap")))
    out.append(("points start in the last 16 bytes of the records", n, [BASE + n * 32 - 16, BASE], ERR_INVALID_ARG, ("range 0", "range 1", "overlap")))
    out.append(("in place", n, [BASE, BASE], ERR_INVALID_ARG, ("overlap",)))
    out.append(("2^62 points", 1 << 62, apart, ERR_INVALID_ARG, ("range 0", "address space")))
    out.append(("2^59 points: only the records wrap", 1 << 59, apart, ERR_INVALID_ARG, ("range 1", "address space")))
    for i, (stride, align) in enumerate(LAYOUT):
        fits = (TOP - 1 - n * stride) // align * align
        for b_i, code in ((fits, OK), (fits + align, ERR_INVALID_ARG)):
            b = list(apart)
            b[i] = b_i
            out.append(("range %d at 2^64 - %d" % (i, TOP - b_i), n, b, code, ("range %d" % i, "address space") if code else ()))
    return out


def test_query_ranges_of_the_call(native_lib):
    strides, aligns = (C.c_uint64 * 2)(*[s for s, _ in LAYOUT]), (C.c_uint32 * 2)(*[a for _, a in LAYOUT])
    table = range_cases()
    assert len(table) > 15
    for label, n, bases, code, words in table:
        assert native_lib.cap_debug_query_ranges(n, 2, (C.c_uint64 * 2)(*bases), strides, aligns) == code, (label, native_lib.cap_last_error())
        message = native_lib.cap_last_error().decode()
        if code:
            assert all(w in message for w in words), (label, message)
