"""Triangle overlap queries without a GPU (cap_overlap_triangles): the prototype, export and binding; the float32 predicate of
tests/overlap_triangles_support.py pinned by hand, held to an exact integer test on the lattice and to its float64 twin on three float
scenes; the walk's prune against each triangle's own vertex box; the address checks of the three ranges; and the inputs of
tests/test_overlap_triangles_gpu.py: each of its cases reaches what it is named after."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import around, needles, soup
from multi_hit_support import stacked_quads
from overlap_triangles_support import (AXES, MISS, NONE, TriTable, all_miss, contact_case, cursors_of, degenerate, exact_meets, far_case, fill_classes, fill_scale,
                                       lattice_case, meets32, meets64, needle_case, node_skipped, pages, queries_of, queries_of_tris, scene_slack, skips_of,
                                       soup_table, tris_around, vertices_of, which_axes)
from test_query_ranges import ERR_INVALID_ARG, OK, disjoint, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
IN_PLANE = set(AXES[11:])    # cross(n, f_i) and cross(m, g_j)
EDGE_EDGE = set(AXES[2:11])  # cross(f_i, g_j)


def one(query, scene):
    return bool(meets32(queries_of_tris([query]), np.asarray([scene], f32))[0, 0])


# 1. the surface
def test_prototype_export_and_binding(native_lib):
    text = open(os.path.join(ROOT, "include", "capsaicin_hip.h")).read()
    assert re.search(r"int cap_overlap_triangles\(CapContext\* ctx, const CapTriangleDesc\* device_queries, uint64_t n, uint32_t k,\s*uint32_t\* device_triangles", text)
    assert hasattr(native_lib, "cap_overlap_triangles") and "cap_overlap_triangles" in capi.SYMBOLS
    T = capi.TriangleDesc
    assert C.sizeof(T) == 48 and (T.a.offset, T.skip.offset, T.b.offset, T.c.offset) == (0, 12, 16, 32)
    assert callable(capi.Renderer.overlap_triangles) and callable(capi.Renderer.scene_triangle_queries)
    assert native_lib.cap_overlap_triangles(None, None, 0, 1, None, None, 0, None) == ERR_INVALID_ARG and b"ctx is NULL" in native_lib.cap_last_error()


def test_triangle_queries_packs_the_rows():
    a, b, c = np.arange(6, dtype=f32).reshape(2, 3), np.arange(6, 12, dtype=f32).reshape(2, 3), np.arange(12, 18, dtype=f32).reshape(2, 3)
    q = capi.Renderer.triangle_queries(a, b, c)
    assert q.shape == (2, 12) and q.dtype == f32 and skips_of(q).tolist() == [NONE, NONE]
    assert np.array_equal(vertices_of(q), np.stack([a, b, c], 1))
    assert skips_of(capi.Renderer.triangle_queries(a, b, c, skip=[7, 0xFFFFFFFE])).tolist() == [7, 0xFFFFFFFE]
    assert np.array_equal(vertices_of(queries_of(a, b, c, [1, 2])), vertices_of(q)) and skips_of(queries_of(a, b, c, [1, 2])).tolist() == [1, 2]
    with pytest.raises(capi.CapError):
        capi.Renderer.triangle_queries(a, b, c[:1])
    with pytest.raises(capi.CapError):
        capi.Renderer.triangle_queries(a, b, c, skip=[1])


# 2. the predicate by hand
def test_contacts_on_the_stacked_quads_by_hand():
    for twice in (False, True):
        tris, names, queries, want = contact_case(twice)
        tab = TriTable(queries, tris)
        for i, (name, ids) in enumerate(zip(names, want)):
            assert tab.candidates(i).tolist() == ids, name
        assert sum(len(w) == 0 for w in want) >= 10 and max(len(w) for w in want) == len(tris)


def test_which_axes_decide():
    _, tris = stacked_quads(8, 0.25)
    inside_lower = [(0.5, 0.125, 0.5), (0.875, 0.125, 0.5), (0.875, 0.375, 0.5)]
    # coplanar with quad 2, inside its lower triangle: from the upper one (id 5) only the in-plane edge normals separate it
    coord, names = which_axes(inside_lower, tris[5])
    assert not coord and names and set(names) <= IN_PLANE, names
    assert which_axes(inside_lower, tris[4]) == (False, [])
    # parallel tilted planes z = x + y and z = x + y + 1, the vertex boxes meet: both normals separate, no in-plane axis does
    tilted = [(0, 0, 0), (4, 0, 4), (0, 4, 4)]
    coord, names = which_axes([(x, y, z + 1) for x, y, z in tilted], tilted)
    assert not coord and {"n", "m"} <= set(names) and not set(names) & IN_PLANE, names
    assert one(tilted, tilted) and not one([(x, y, z + 1) for x, y, z in tilted], tilted)
    # a pair of the lattice that only an edge-edge axis separates: the vertex boxes meet, each plane cuts the other triangle
    q, t = [(8, 4, 0), (-4, -1, 0), (-1, 3, 0)], [(-3, 6, 1), (3, 0, 0), (0, 4, 1)]
    coord, names = which_axes(q, t)
    assert not coord and names == ["f0 x g0"] and not exact_meets(q, t) and not one(q, t)
    assert set(names) <= EDGE_EDGE
    # beside the vertex box: a coordinate axis
    assert which_axes([(1.5, 1.5, 0), (2, 2, 2), (2, 1.5, 1)], tris[0])[0]


def test_points_segments_and_the_conservative_case():
    tri = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
    # a point in the face, on an edge, on a vertex; off the plane; in the plane beside the hypotenuse (inside the vertex box)
    assert one([(1, 1, 0)] * 3, tri) and one([(2, 2, 0)] * 3, tri) and one([(4, 0, 0)] * 3, tri)
    assert not one([(1, 1, 0.5)] * 3, tri) and not one([(3, 3, 0)] * 3, tri)
    coord, names = which_axes([(3, 3, 0)] * 3, tri)
    assert not coord and set(names) <= IN_PLANE, "a point in the plane is decided by cross(m, g_j)"
    # a segment through the face, one that ends in it, one that passes beside the hypotenuse inside the vertex box, one in the plane
    assert one([(1, 1, -1), (1, 1, 1), (1, 1, 1)], tri) and one([(1, 1, 0), (1, 1, 1), (1, 1, 1)], tri)
    assert not one([(3, 3, -1), (3, 3, 1), (3, 3, 1)], tri)
    assert one([(-1, 1, 0), (5, 1, 0), (5, 1, 0)], tri) and not one([(3, 2, 0), (2, 3, 0), (2, 3, 0)], tri)
    # two coplanar segments that do not cross, with vertex boxes that meet, are LISTED: every axis of the pair is zero or along the
    # common normal.  Documented in the header; asserted so that it stays so.
    a, b = [(0, 0, 0), (2, 2, 0), (2, 2, 0)], [(1, 0, 0), (2, 0.5, 0), (2, 0.5, 0)]
    assert one(a, b) and one(b, a)
    assert which_axes(a, b) == (False, [])


def test_non_finite_queries_are_not_traversed():
    tris = np.array([[(0, 0, 0), (1, 0, 0), (0, 1, 0)]], f32)
    nan, inf = np.nan, np.inf
    q = queries_of_tris(np.array([[(0.25, 0.25, -1), (0.25, 0.25, 1), (0.5, 0.25, 1)], [(nan, 0.25, -1), (0.25, 0.25, 1), (0.5, 0.25, 1)],
                                  [(0.25, 0.25, -1), (0.25, inf, 1), (0.5, 0.25, 1)], [(0.25, 0.25, -1), (0.25, 0.25, 1), (0.5, 0.25, -inf)],
                                  [(-inf, -inf, -inf), (inf, inf, inf), (inf, -inf, 0)]], f32))
    assert degenerate(q).tolist() == [False, True, True, True, True]
    tab = TriTable(q, tris)
    page, cnt = tab.page(2)
    assert page[0].tolist() == [0, MISS] and (page[1:] == MISS).all() and cnt.tolist() == [1, 0, 0, 0, 0]
    assert (tab.page(2, cursors_of(page))[0] == MISS).all()


def test_skip_is_applied_like_the_mask():
    tris, _, _, _ = contact_case()
    q = queries_of_tris(tris[[4, 4, 4]], skip=[4, NONE, 1000])
    tab = TriTable(q, tris)
    assert tab.candidates(0).tolist() == [5] and tab.candidates(1).tolist() == [4, 5] and tab.candidates(2).tolist() == [4, 5]
    assert tab.counts().tolist() == [1, 2, 2]


# 3. the lattice: float32 is exact there
def test_lattice_float32_float64_and_the_exact_test_agree():
    """Integer coordinates |x| <= 8: every intermediate value is an integer below 3 * 2^18 < 2^24, so float32 computes the predicate of
    the reals, and for triangles of non-zero area that is the truth."""
    scene, queries, exact = lattice_case()
    q = queries_of_tris(queries)
    m32, m64 = meets32(q, scene.astype(f32)), meets64(q, scene.astype(f32))
    print("lattice: %d pairs, %d overlap; float32 differs from the exact test on %d, float64 on %d"
          % (exact.size, exact.sum(), (m32 != exact).sum(), (m64 != exact).sum()))
    assert exact.size >= 30000 and exact.sum() >= exact.size // 4
    assert np.array_equal(m32, exact) and np.array_equal(m64, exact)
    planar = (queries[:, :, 2] == 0).all(1)[:, None] & (scene[:, :, 2] == 0).all(1)[None]
    assert planar.sum() > 2000 and exact[planar].any() and not exact[planar].all(), "coplanar pairs of both kinds"
    # on the lattice the predicate is symmetric: the other triangle's frame gives the same answer
    assert np.array_equal(meets32(queries_of_tris(scene), queries.astype(f32)).T, m32)


def test_exact_test_by_hand():
    t = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
    assert exact_meets(t, [(1, 1, -1), (1, 1, 1), (2, 1, 1)]) and exact_meets(t, [(1, 1, 0), (1, 1, 1), (2, 1, 1)])  # through, touching
    assert not exact_meets(t, [(1, 1, 1), (1, 2, 1), (2, 1, 1)]) and not exact_meets(t, [(3, 3, -1), (3, 3, 1), (4, 4, 1)])
    assert exact_meets(t, [(1, 1, 0), (2, 1, 0), (1, 2, 0)]) and exact_meets([(1, 1, 0), (2, 1, 0), (1, 2, 0)], t)  # coplanar, contained
    assert exact_meets(t, [(4, 0, 0), (6, 0, 0), (6, 2, 0)]) and exact_meets(t, [(2, 2, 0), (4, 4, 0), (2, 4, 0)])  # a shared vertex; a vertex on an edge
    assert not exact_meets(t, [(3, 2, 0), (5, 2, 0), (3, 4, 0)]) and exact_meets(t, [(-1, -1, 0), (9, -1, 0), (-1, 9, 0)])  # coplanar beside; around
    assert exact_meets(t, [(4, 0, 0), (0, 4, 0), (4, 4, 3)]) and not exact_meets(t, [(4, 1, 0), (1, 4, 0), (4, 4, 3)])  # a shared edge; just off it


# 4. float32 against float64 on float scenes, and the prune
def twin_scenes():
    rng = np.random.default_rng(29)
    quads = stacked_quads(40, 0.025)[1]
    for name, tris, edge in (("soup", soup(rng, 3000, edge=0.2), 1.0), ("needles", needles(rng, 3000, aspect=1e4), 1.0),
                             ("stacked_quads", np.asarray(quads, f32), 1.5)):
        centres = around(rng, tris, 512, 0.05)
        yield name, np.asarray(tris, f32), queries_of_tris(tris_around(rng, centres, rng.random(512) * edge))


def test_float32_against_the_float64_twin_and_the_prune():
    """The number of pairs on which float32 and float64 disagree is a CPU observation, printed and quoted in DESIGN.md, not held to a
    cap.  Asserted: with each triangle's own vertex box standing for every node box above it (those only contain it), no pair that
    meets32 lists is skipped by the walk's test against the box of the query's vertices grown by the slack."""
    for name, tris, queries in twin_scenes():
        m32, m64 = meets32(queries, tris), meets64(queries, tris)
        print("%s: %d pairs, %d overlap, %d differ from float64" % (name, m32.size, m32.sum(), (m32 != m64).sum()))
        assert m32.sum() > 300, name
        tl, th = tris.min(1), tris.max(1)
        A = vertices_of(queries)
        slack = scene_slack(tris)
        skipped = np.stack([node_skipped(tl, th, a.min(0), a.max(0), slack) for a in A])
        assert not (skipped & m32).any(), "%s, slack %g: an overlapping pair is skipped" % (name, slack)
        assert skipped.sum() > 0.5 * skipped.size, "the prune prunes"


# 5. the three ranges
def test_address_checks_of_the_three_ranges(native_lib):
    n, k = 8, 3  # (eight: every array's length is a multiple of 16, so disjoint()'s bases are aligned)
    layout = [(48, 16), (4 * k, 4), (4, 4)]  # queries, ids, counts
    strides, aligns = [s for s, _ in layout], [a for _, a in layout]
    base = disjoint(layout, n)
    assert run(native_lib, n, base, strides, aligns) == OK
    for i, offs in ((0, (4, 8, 12)), (1, (1, 2, 3)), (2, (1, 2, 3))):
        for off in offs:
            b = list(base)
            b[i] += off
            assert run(native_lib, n, b, strides, aligns) == ERR_INVALID_ARG and b"aligned" in native_lib.cap_last_error()
    for i in range(3):
        for j in range(3):
            if i != j:
                b = list(base)
                b[j] = b[i] + (n - 1) * layout[i][0] // 16 * 16  # range j starts near range i's end, aligned for every j
                assert run(native_lib, n, b, strides, aligns) == ERR_INVALID_ARG and b"overlap" in native_lib.cap_last_error()
    b = list(base)
    b[1] = b[0] + 1  # k = 0: the page is left out, wherever its pointer points
    assert run(native_lib, n, b, [48, 0, 4], aligns) == OK
    assert run(native_lib, 1 << 60, base, [48, 0, 0], aligns) == ERR_INVALID_ARG and b"address space" in native_lib.cap_last_error()
    assert run(native_lib, 1 << 58, base, [0, 4 * 16, 0], aligns) == ERR_INVALID_ARG and b"address space" in native_lib.cap_last_error()


# 6. the GPU cases reach what they are named after
@pytest.mark.parametrize("k", (1, 2, 4, 5, 8, 9, 16))
def test_fill_classes_of_the_soup(k):
    classes = fill_classes(soup_table(fill_scale(k)).counts(), k)
    assert min(classes) >= 5 and min(classes[:3]) >= 20, "k = %d: queries with 0, 1..k, k+1..3k and more candidates: %s" % (k, classes)


def test_cursor_rule_walks_every_candidate_once():
    tab = soup_table(0.8).first(64)
    cnt = tab.counts().astype(np.int64)
    assert cnt.max() > 16
    for k in (1, 3, 16):
        seq = pages(tab, k)
        assert all_miss(seq[-1][0]) and len(seq) == -(-int(cnt.max()) // k) + 1, "the page after a short or a just-full page is empty"
        for i in range(tab.n):
            got = np.concatenate([p[i][p[i] != MISS] for p, _ in seq])
            assert got.tolist() == tab.candidates(i).tolist()


def test_far_and_needle_cases_have_candidates_and_near_misses():
    for case in (far_case, needle_case):
        tris, tab = case()
        cnt = tab.counts()
        assert (cnt > 0).sum() >= 40 and (cnt == 0).sum() >= 20 and cnt.max() >= 8, (case.__name__, (cnt > 0).sum(), (cnt == 0).sum(), cnt.max())
        # queries whose vertex box meets a triangle's and that do not meet the triangle: what only the seventeen axes tell apart
        tl, th = tris.min(1), tris.max(1)
        boxes_meet = np.stack([~node_skipped(tl, th, a.min(0), a.max(0), 0) for a in vertices_of(tab.b)])
        assert (boxes_meet & ~tab.meets).sum() >= 40, case.__name__
