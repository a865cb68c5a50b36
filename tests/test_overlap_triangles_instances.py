"""Triangle overlap queries over instances without a GPU (cap_overlap_triangles_instances): the prototype, the export and the binding;
the float32 reference of overlap_triangles_instances_support.py pinned by hand and by the contract's three identities, printed against
its float64 twin; the walk's world-node prune asked through cap_debug_overlap_world_node for every candidate pair; the scene built to
defeat the object-space prune of cap_overlap_instances; the address checks of the call's four arrays; and that the cases of
tests/test_overlap_triangles_instances_gpu.py reach what they are named after."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_instances_support import live_of, world_records
from closest_point_support import arrays, records_of, soup
from instance_support import extreme_transforms, grid_scene, regular_transforms, translations
from overlap_instances_support import model_image, model_miss, prune
from overlap_triangles_instances_support import (C2, MISS, NONE, TriPairTable, affine, all_miss, contact_instances, counterexample, cursors_of, far_case,
                                                 fill_classes, identity, meets_pairs, model_world_box, model_world_skip, needle_case, odd_queries, pages,
                                                 pair_valid, queries_near, queries_of, queries_of_tris, query_boxes, regular_case, skip_instances_of,
                                                 skips_of, soup_case, vertices_of, with_skip_pair, world_node)
from overlap_triangles_support import TriTable, soup_table
from overlap_triangles_support import soup_scene as flat_soup_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID_ARG = 0, 1
f32 = np.float32


# ---- prototype, export, binding ----
def test_header_prototype_compiles(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "overlap_triangles_instances.c"
    src.write_text("""#include <stddef.h>
#include "capsaicin_hip.h"
_Static_assert(sizeof(CapTriangleDesc) == 48 && offsetof(CapTriangleDesc, skip) == 12 && offsetof(CapTriangleDesc, pad0) == 28, "the record did not move");
int (*const overlap)(CapContext*, const CapTriangleDesc*, uint64_t, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t,
                     const CapTraceOptions*) = cap_overlap_triangles_instances;
int (*const node)(const float*, const float*, const float*, const float*, const float*, const float*, const float*, float*, float*, float*, float*,
                  uint32_t*) = cap_debug_overlap_world_node;
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "o.o")])


def test_entry_points_are_exported_and_bound(native_lib):
    assert hasattr(native_lib, "cap_overlap_triangles_instances") and hasattr(native_lib, "cap_debug_overlap_world_node")
    assert len(capi.SYMBOLS["cap_overlap_triangles_instances"][1]) == 9 and len(capi.SYMBOLS["cap_debug_overlap_world_node"][1]) == 12
    assert callable(capi.Renderer.overlap_triangles_instances) and callable(capi.Renderer.instance_triangle_queries)
    assert native_lib.cap_overlap_triangles_instances(None, None, 0, 1, None, None, None, 0, None) == ERR_INVALID_ARG
    assert b"cap_overlap_triangles_instances: ctx is NULL" in native_lib.cap_last_error()
    assert native_lib.cap_debug_overlap_world_node(*([None] * 12)) == ERR_INVALID_ARG


def test_triangle_queries_with_skip_instance():
    a, b, c = np.arange(6, dtype=f32).reshape(2, 3), np.arange(6, 12, dtype=f32).reshape(2, 3), np.arange(12, 18, dtype=f32).reshape(2, 3)
    q = capi.Renderer.triangle_queries(a, b, c)
    assert skips_of(q).tolist() == [NONE, NONE] and skip_instances_of(q).tolist() == [0, 0], "the default leaves column 7 at 0, as before"
    q = capi.Renderer.triangle_queries(a, b, c, skip=[7, 9], skip_instance=[3, 0xFFFFFFFE])
    assert skips_of(q).tolist() == [7, 9] and skip_instances_of(q).tolist() == [3, 0xFFFFFFFE] and not q.view(np.uint32)[:, 11].any()
    assert np.array_equal(vertices_of(q), np.stack([a, b, c], 1))
    assert np.array_equal(q.view(np.uint32), with_skip_pair(capi.Renderer.triangle_queries(a, b, c), [3, 0xFFFFFFFE], [7, 9]).view(np.uint32))
    with pytest.raises(capi.CapError):
        capi.Renderer.triangle_queries(a, b, c, skip=[1, 2], skip_instance=[1])


def host_renderer(tris):
    """a Renderer without a context: what instance_triangle_queries reads is the wrapper's host copy of the scene"""
    r = capi.Renderer.__new__(capi.Renderer)
    a = arrays(tris)
    r.ctx = None
    r._set_mesh_table(a[4])
    r._scene_host = (np.asarray(a[0], f32).reshape(-1, 3).copy(), np.asarray(a[3], np.uint32).ravel().copy(), np.asarray(a[4], np.uint32).reshape(-1, 8).copy())
    return r


def test_instance_triangle_queries_are_the_world_records():
    rng = np.random.default_rng(2)
    tris = soup(rng, 50, edge=0.3)
    M = regular_transforms(7)
    inst, ids = rng.integers(0, 7, 40), rng.integers(0, 50, 40)
    q = host_renderer(tris).instance_triangle_queries(M, inst, ids)
    v0w, e1w, e2w = world_records(M, tris)
    want = np.stack([v0w[inst, ids], v0w[inst, ids] + e1w[inst, ids], v0w[inst, ids] + e2w[inst, ids]], 1)
    assert q.dtype == f32 and np.array_equal(vertices_of(q).view(np.uint32), want.view(np.uint32)), "bit for bit the contract's computed vertices"
    assert skips_of(q).tolist() == ids.tolist() and skip_instances_of(q).tolist() == inst.tolist()
    # every placed triangle meets itself; the skip pair takes exactly that pair out
    tab, plain = TriPairTable(q, M, tris), TriPairTable(with_skip_pair(q, np.zeros(40), np.full(40, NONE)), M, tris)
    for n in range(40):
        assert (int(inst[n]), int(ids[n])) in plain.pairs(n) and [p for p in plain.pairs(n) if p != (int(inst[n]), int(ids[n]))] == tab.pairs(n)
    with pytest.raises(capi.CapError):
        host_renderer(tris).instance_triangle_queries(M, [7], [0])
    with pytest.raises(capi.CapError):
        host_renderer(tris).instance_triangle_queries(M, [0, 1], [0])


# ---- the reference by hand ----
def test_contacts_under_a_translation_and_a_stretch():
    tris, M, names, q, want = contact_instances()
    tab = TriPairTable(q, M, tris)
    assert sum(1 for p in want if not p) >= 20 and sum(1 for n in names if "one ulp" in n) == 14
    for n, (name, pairs) in enumerate(zip(names, want)):
        assert tab.pairs(n) == pairs, (name, tab.pairs(n), pairs)


def test_the_skip_pair():
    tris, M, names, q, want = contact_instances()
    everything = names.index("translated: everything")
    assert want[everything] == [(0, g) for g in range(16)]
    row = q[everything:everything + 1]
    for pair, gone in (((0, 5), [(0, 5)]), ((1, 5), []), ((0, 16), []), ((2, 5), []), ((0, NONE), []), ((NONE, NONE), []), ((0, 0), [(0, 0)]), ((NONE, 5), [])):
        got = TriPairTable(with_skip_pair(row, [pair[0]], [pair[1]]), M, tris).pairs(0)
        assert got == [p for p in want[everything] if p not in gone], (pair, got)
    # skip = 0xFFFFFFFF with pad0 = 0 skips nothing -- not even the pair (0, 0xFFFFFFFF & anything): zeroed pads stay harmless
    zeroed = capi.Renderer.triangle_queries(*(vertices_of(row)[:, j] for j in range(3)))
    assert skips_of(zeroed).tolist() == [NONE] and skip_instances_of(zeroed).tolist() == [0]
    assert TriPairTable(zeroed, M, tris).pairs(0) == want[everything]
    # the pair is applied like the mask: it is not counted, and the cursor passes over it
    tab = TriPairTable(with_skip_pair(row, [0], [5]), M, tris)
    assert tab.counts()[0] == 15 and tab.pairs(0, (0, 4)) == [(0, g) for g in range(6, 16)]


def test_inert_masked_instances_and_objects():
    tris = soup(np.random.default_rng(7), 60, edge=0.3)
    M, must_be_inert = extreme_transforms()
    M = np.concatenate([M, regular_transforms(3)])
    live = live_of(M)
    assert not live[:len(must_be_inert)][must_be_inert].any() and live.sum() >= 4
    # a query that is every placed triangle's own: each live instance answers with at least that triangle
    lv = np.nonzero(live)[0]
    q = host_renderer(tris).instance_triangle_queries(M, np.repeat(lv, 3), np.tile([0, 30, 59], len(lv)))
    q = with_skip_pair(q, np.zeros(len(q)), np.full(len(q), NONE))
    with np.errstate(all="ignore"):
        tab = TriPairTable(q, M, tris)
    valid = pair_valid(len(M), 60, live)
    t = tab.with_valid(valid)
    for n in range(len(q)):
        assert (int(lv[n // 3]), [0, 30, 59][n % 3]) in t.pairs(n) and all(live[i] for i, _ in t.pairs(n))
    im = np.full(len(M), 0xFF, np.uint32)
    im[lv[0]] = 0x02
    masked = tab.with_valid(pair_valid(len(M), 60, live, im, None, 0x01))
    assert all(i != lv[0] for n in range(len(q)) for i, _ in masked.pairs(n)) and masked.counts()[3:].sum() > 0
    mesh = tab.with_valid(pair_valid(len(M), 60, live, None, np.where(np.arange(60) < 30, 0x01, 0x02), 0x02))
    assert all(g >= 30 for n in range(len(q)) for _, g in mesh.pairs(n)) and mesh.counts().sum() > 0
    obj = tab.with_valid(pair_valid(len(M), 60, live, None, None, None, np.arange(len(M)) % 2, (np.arange(60) >= 20).astype(int)))
    assert all((g >= 20) == (i % 2 == 1) for n in range(len(q)) for i, g in obj.pairs(n)) and 0 < obj.counts().sum() < t.counts().sum()


def test_coincident_instances_page_every_pair_once_in_order():
    tris = soup(np.random.default_rng(5), 40, edge=0.3)
    M = np.stack([identity()[0], identity()[0], affine(np.eye(3), (8, 0, 0)), identity()[0]])
    tab = TriPairTable(queries_near(np.random.default_rng(6), M[:1], tris, 32, size=1.5, away=1000), M, tris)
    flat = TriTable(tab.b, tris)
    for n in range(32):
        assert tab.pairs(n) == [(i, int(g)) for i in (0, 1, 3) for g in flat.candidates(n)]
    for k in (1, 3, 16):
        walk = pages(tab, k)
        assert all_miss(walk[-1][0]) and all_miss(walk[-1][1]) and not all_miss(walk[-2][0])
        for n in range(32):
            tri, inst = np.concatenate([p[0][n] for p in walk]), np.concatenate([p[1][n] for p in walk])
            assert ((tri == MISS) == (inst == MISS)).all()
            assert (inst[inst != MISS].astype(np.int64) * 40 + tri[tri != MISS]).tolist() == tab.candidates(n).tolist()
        assert (walk[0][2] == tab.counts()).all() and (walk[-1][2] == 0).all()
    assert len(tab.candidates(0, (MISS, MISS))) == 0 and len(tab.candidates(0, (3, 39))) == 0, "the cursor of a short page admits nothing"


# ---- the three identities ----
def test_one_identity_instance_is_the_flat_query():
    tris = flat_soup_scene()[0][:800]
    q = np.concatenate([soup_table(0.8).b[:64], queries_of_tris(tris[:64])])  # the second half meet themselves
    ids = np.concatenate([np.arange(64) + 100, np.arange(64)])
    flat = TriTable(with_skip_pair(q, np.zeros(128), ids), tris)
    tab = TriPairTable(with_skip_pair(q, np.zeros(128), ids), identity(), tris)  # skip_instance = 0
    assert np.array_equal(tab.meets, flat.meets) and flat.meets.any()
    assert not np.array_equal(TriPairTable(q, identity(), tris).meets, tab.meets), "the skip pair took something out"
    for w, o in zip((x[0] for x in world_records(identity(), tris)), records_of(tris)):
        assert np.array_equal(w, o)


def test_translations_on_a_grid_give_the_flattened_scene():
    rng = np.random.default_rng(8)
    _, tris = grid_scene()
    T = rng.integers(-32 * 16, 32 * 16 + 1, (6, 3)) / 16.0
    M = translations(T)
    flat_tris = np.concatenate([(tris.astype(np.float64) + t).astype(f32) for t in T])
    assert np.array_equal(flat_tris.astype(np.float64), np.concatenate([tris.astype(np.float64) + t for t in T])), "every sum is exact"
    q = grid_queries(rng, T)
    tab, flat = TriPairTable(q, M, tris), TriTable(q, flat_tris)
    assert np.array_equal(tab.meets, flat.meets) and 0 < tab.meets.sum() < tab.meets.size
    assert len(np.unique(tab.inst_of[np.nonzero(tab.meets.any(0))[0]])) == 6


def grid_queries(rng, T, n=96):
    """query triangles on the grid of sixteenths around the translations"""
    c = T[rng.integers(0, len(T), n)] + rng.integers(-8 * 16, 8 * 16 + 1, (n, 3)) / 16.0
    v = c[:, None, :] + rng.integers(-4 * 16, 4 * 16 + 1, (n, 3, 3)) / 16.0
    assert np.array_equal(v.astype(f32).astype(np.float64), v)
    return queries_of_tris(v.astype(f32))


def test_scaling_by_a_power_of_two_changes_nothing():
    tris, M, tab = soup_case()
    for j in (-20, 7):
        s = f32(2.0 ** j)
        scaled = tab.b[:64].copy()
        scaled[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] *= s
        assert np.array_equal(meets_pairs(scaled, (M * s).astype(f32), tris), meets_pairs(tab.b[:64], M, tris))


# ---- the float64 twin: printed, held to no cap ----
def test_the_reference_against_its_float64_twin():
    tris, M, tab = regular_case()
    twin = meets_pairs(tab.b, M, tris, np.float64)
    differ = int((twin != meets_pairs(tab.b, M, tris)).sum())
    print("soup under regular_transforms(32): %d of %d pairs differ from the float64 twin, %d candidates" % (differ, twin.size, int(tab.meets.sum())))


# ---- the prune never skips a candidate: a condition, not a tolerance ----
def candidate_skips(tris, M, tab, live=None, c2=None):
    """(pairs asked, skipped) for every candidate pair of the table, the triangle's own float32 vertex box standing for the node boxes
    above it.  c2 = None: through the debug entry, which the numpy model must equal on every pair; else the model with that constant."""
    lib = capi.lib()
    olo, ohi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    nlo, nhi = tris.min(1), tris.max(1)
    qlo, qhi = query_boxes(tab.b)
    asked = skipped = 0
    for i in range(tab.i):
        if live is not None and not live[i]:
            continue
        qs, gs = np.nonzero(tab.meets[:, i * tab.t:(i + 1) * tab.t])
        if len(qs) == 0:
            continue
        xw = world_node(M[i], olo, ohi, nlo[gs[0]], nhi[gs[0]], qlo[qs[0]], qhi[qs[0]], lib)["xw"]
        model = model_world_skip(M[i], xw, nlo[gs], nhi[gs], qlo[qs], qhi[qs], C2 if c2 is None else c2)
        if c2 is None:
            for n, (q, g) in enumerate(zip(qs, gs)):
                p = world_node(M[i], olo, ohi, nlo[g], nhi[g], qlo[q], qhi[q], lib)
                assert p["skip_node"] == int(model[n]), "the model is the shipped arithmetic"
                skipped += p["skip_node"]
        else:
            skipped += int(model.sum())
        asked += len(qs)
    return asked, skipped


PRUNE_CASES = (regular_case, far_case, needle_case)


@pytest.mark.parametrize("case", PRUNE_CASES, ids=("soup", "near 4096", "needles"))
def test_the_world_node_prune_skips_no_candidate(native_lib, case):
    tris, M, tab = case()
    asked, skipped = candidate_skips(tris, M, tab)
    print("%s: %d candidate pairs, %d skipped at the node" % (case.__name__, asked, skipped))
    assert asked > 1500 and skipped == 0


def test_the_world_node_prune_skips_no_candidate_of_extreme_transforms(native_lib):
    tris = soup(np.random.default_rng(42), 120, edge=0.2)
    M, _ = extreme_transforms()
    live = live_of(M)
    q = np.concatenate([queries_near(np.random.default_rng(43), M[live], tris, 256, size=1.0), odd_queries()])
    with np.errstate(all="ignore"):
        tab = TriPairTable(q, M, tris)
        asked, skipped = candidate_skips(tris, M, tab, live)
    assert asked > 300 and skipped == 0


def test_what_the_prune_loses_without_the_slack(native_lib):
    """The same question of the model with the constant forced to 0.  Reported, not asserted: with the triangle's own vertex box
    standing for the node boxes, the world box of that box is so much larger than the triangle's world record (by the rotation, and by
    h_w >= the record's own extent otherwise) that no scene here loses a candidate even without the slack -- 0, 0 and 0 when this was
    written, and 0 of 1 983 under pure translations near 4 096 (DESIGN.md says so).  With the shipped constant nothing may be lost."""
    lost = {}
    for case in PRUNE_CASES:
        tris, M, tab = case()
        lost[case.__name__] = candidate_skips(tris, M, tab, c2=0.0)[1]
        assert candidate_skips(tris, M, tab, c2=C2)[1] == 0
    print("without the slack the model skips %s candidates" % lost)


def test_the_debug_entry_reports_the_world_box(native_lib):
    for M in regular_transforms(12):
        p = world_node(M, (0, 0, 0), (1, 1, 1), (0.25, 0, 0.5), (1, 0.75, 1), (-1, -2, -3), (4, 5, 6))
        assert p["xw"] >= np.abs(M[:, 3]).max() and f32(p["slack"]) == (C2 * f32(2.0 ** -24)) * (f32(6.0) + f32(p["xw"]))
        wlo, whi = model_world_box(M, f32([0.25, 0, 0.5]), f32([1, 0.75, 1]))
        assert np.array_equal(wlo, p["world_lo"]) and np.array_equal(whi, p["world_hi"])
        # the world box holds the exact images of the node's corners, to the 11 eps Xw of the argument
        corners = np.array([[(1, 0.75, 1)[k] if (c >> k) & 1 else (0.25, 0, 0.5)[k] for k in range(3)] for c in range(8)], np.float64)
        w = corners @ M[:, :3].astype(np.float64).T + M[:, 3].astype(np.float64)
        tol = 11 * 2.0 ** -24 * p["xw"]
        assert (w >= wlo - tol).all() and (w <= whi + tol).all() and (w.min(0) <= wlo + tol).all() and (w.max(0) >= whi - tol).all()
    inert = world_node(np.zeros((3, 4), f32), (0, 0, 0), (1, 1, 1), (5, 5, 5), (6, 6, 6), (0, 0, 0), (1, 1, 1))
    assert inert["xw"] == 0 and inert["slack"] == 0 and inert["skip_node"] == 0 and not inert["world_lo"].any() and not inert["world_hi"].any()
    far = world_node(identity()[0], (0, 0, 0), (6, 6, 6), (5, 5, 5), (6, 6, 6), (0, 0, 0), (1, 1, 1))
    assert far["skip_node"] == 1
    touch = world_node(identity()[0], (0, 0, 0), (6, 6, 6), (1, 1, 1), (6, 6, 6), (0, 0, 0), (1, 1, 1))
    assert touch["skip_node"] == 0
    nan = world_node(affine(np.eye(3) * 1e30), (0, 0, 0), (3e38, 1, 1), (-3e38, 0, 0), (3e38, 1, 1), (0, 0, 0), (1, 1, 1))
    assert nan["skip_node"] == 0, "a world box that is not finite opens the node"


# ---- the scene built to defeat the object-space prune ----
def test_the_counterexample_defeats_the_image_prune_and_not_the_world_prune(native_lib):
    tris, M, q = counterexample()
    tab = TriPairTable(q, M, tris)
    assert tab.pairs(0) == [(0, 0)], "two coplanar segments that do not cross: listed by the contract, and nothing else is"
    far = np.abs(tris[1:].astype(np.float64) - tris[0].astype(np.float64).mean(0)).max(-1).min()
    assert far >= 10.0, "the fillers lie at least 10 units away"
    olo, ohi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    qlo, qhi = query_boxes(q)
    # the box query's prune on the query's bounding box: its object-space image misses the segment's own vertex box
    p = prune(M[0], olo, ohi, olo, ohi, tris[0].min(0), tris[0].max(0), qlo[0], qhi[0])
    slack, ilo, ihi = model_image(p["W"], p["g"], p["xw"], qlo[0], qhi[0])
    assert np.array_equal(ilo, p["image_lo"]) and ilo[0] > -1e-3 and tris[0, :, 0].max() < -1.41
    assert model_miss(tris[0].min(0), tris[0].max(0), ilo, ihi) and p["skip_node"] == 1, "cap_overlap_instances' prune would skip the segment"
    # ... and so would it skip an inner node above the segment in the tree the host builder makes of this scene
    nodes, order, depth = capi.host_sah_build(tris.min(1), tris.max(1))
    above = []
    for row in nodes:
        for lo, hi in ((row[0:3], row[3:6]), (row[6:9], row[9:12])):
            if (lo <= tris[0].min(0)).all() and (hi >= tris[0].max(0)).all() and not (lo <= olo).all():
                above.append((lo.copy(), hi.copy()))
    assert len(above) >= 2 and any((hi - lo).max() > 6 for lo, hi in above), "child boxes above the segment, an inner node's among them"
    for lo, hi in above:
        assert model_miss(lo, hi, ilo, ihi), "the image excludes every box above the segment"
        w = world_node(M[0], olo, ohi, lo, hi, qlo[0], qhi[0])
        assert w["skip_node"] == 0 and not model_world_skip(M[0], w["xw"], lo, hi, qlo[0], qhi[0]), "the world-node test keeps it"
    assert world_node(M[0], olo, ohi, tris[0].min(0), tris[0].max(0), qlo[0], qhi[0])["skip_node"] == 0


# ---- the address checks of the call's four arrays ----
BASE = 1 << 40


def layout_of(k):
    """queries, triangle pages, instance pages, counts: (bytes per query, alignment); stride 0 = left out (k = 0)"""
    return ((48, 16), (4 * k, 4), (4 * k, 4), (4, 4))


@pytest.mark.parametrize("k", (1, 16, 0))
def test_query_ranges_of_the_call(native_lib, k):
    layout = layout_of(k)
    strides, aligns = (C.c_uint64 * 4)(*[s for s, _ in layout]), (C.c_uint32 * 4)(*[a for _, a in layout])
    n = 1000
    size = [n * s for s, _ in layout]
    apart = [BASE + (i << 30) for i in range(4)]
    table = [("apart", n, apart, OK, ())]
    for i, (s, a) in enumerate(layout):
        if s:
            b = list(apart)
            b[i] += a // 2
            table.append(("range %d misaligned" % i, n, b, ERR_INVALID_ARG, ("range %d" % i, "aligned")))
    for i in range(4):
        for j in range(4):
            if i == j or not layout[i][0] or not layout[j][0]:
                continue
            b = list(apart)
            b[j] = b[i] + size[i]
            table.append(("range %d right behind range %d" % (j, i), n, b, OK, ()))
            b = list(apart)
            b[j] = b[i] + size[i] - layout[j][1]
            table.append(("range %d starts in the last bytes of range %d" % (j, i), n, b, ERR_INVALID_ARG, ("overlap",)))
    table.append(("2^62 queries", 1 << 62, apart, ERR_INVALID_ARG, ("address space",)))
    assert len(table) >= (30 if k else 8)
    for label, m, bases, code, words in table:
        if k == 0:
            bases = [bases[0], bases[0], bases[3], bases[3]]  # the pages are left out and never looked at, wherever they point
        assert native_lib.cap_debug_query_ranges(m, 4, (C.c_uint64 * 4)(*bases), strides, aligns) == code, (label, native_lib.cap_last_error())
        message = native_lib.cap_last_error().decode()
        if code:
            assert all(w in message for w in words), (label, message)


# ---- the cases of the GPU tests reach what they are named after ----
@pytest.mark.parametrize("k", (1, 2, 4, 5, 8, 9, 16))
def test_fill_classes_of_the_gpu_cases(k):
    _, _, tab = soup_case()
    classes = fill_classes(tab.counts(), k)
    assert min(classes) >= 8, "queries with 0, 1..k, k+1..3k and more pairs: %s" % classes
    _, inst, _ = tab.page(k)
    assert len(np.unique(inst[inst != MISS])) >= 16, "pairs of many instances in the pages"


def test_pages_of_the_soup_span_instances():
    _, _, tab = soup_case()
    _, inst, _ = tab.page(16)
    assert sum(1 for row in inst if len(np.unique(row[row != MISS])) > 1) >= 16, "queries that meet several instances"
    assert len(cursors_of(*tab.page(3)[:2])) == tab.n


def test_odd_queries_are_what_they_are_named():
    q = odd_queries()
    tab = TriPairTable(q, identity(), soup(np.random.default_rng(1), 20, edge=0.5))
    assert tab.bad.tolist() == [False] * 4 + [True] * 4 and tab.counts()[0] > 0 and (tab.counts()[4:] == 0).all()
