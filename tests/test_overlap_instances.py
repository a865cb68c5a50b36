"""Box overlap queries over instances without a GPU (cap_overlap_instances): the prototype, the export and the binding; the float32
reference of overlap_instances_support.py pinned by hand and by the contract's three identities, held to its float64 twin; the walk's
prune asked through cap_debug_overlap_instance_prune for every candidate pair; the address checks of the call's four arrays; and that
the cases of tests/test_overlap_instances_gpu.py reach what they are named after."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_instances_support import live_of, world_records
from closest_point_support import records_of, soup
from instance_support import extreme_transforms, grid_scene, regular_transforms, translations
from overlap_instances_support import (C2, MISS, PairTable, affine, all_miss, boxes_near, boxes_of, cursors_of, far_case, fill_classes, huge_boxes,
                                       identity, meets_pairs, model_image, model_skips, needle_case, pages, pair_valid, prune, soup_case, stand_in_boxes,
                                       touching_instances)
from overlap_support import Table, axes, soup_scene, soup_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID_ARG = 0, 1
f32 = np.float32


def test_header_prototype_compiles(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "overlap_instances.c"
    src.write_text("""#include "capsaicin_hip.h"
_Static_assert(CAP_MULTI_MAX_K == 16 && CAP_MULTI_CONTINUE == 1, "the multi-hit queries' page limit and flag");
_Static_assert(sizeof(CapBoxDesc) == 32, "a box is two float4");
int (*const overlap_instances)(CapContext*, const CapBoxDesc*, uint64_t, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t,
                               const CapTraceOptions*) = cap_overlap_instances;
int (*const prune)(const float*, const float*, const float*, const float*, const float*, const float*, const float*, const float*, const float*,
                   float*, float*, float*, float*, float*, float*, uint32_t*, uint32_t*) = cap_debug_overlap_instance_prune;
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "overlap_instances.o")])


def test_entry_points_are_exported_and_bound(native_lib):
    assert hasattr(native_lib, "cap_overlap_instances") and hasattr(native_lib, "cap_debug_overlap_instance_prune")
    assert len(capi.SYMBOLS["cap_overlap_instances"][1]) == 9 and len(capi.SYMBOLS["cap_debug_overlap_instance_prune"][1]) == 17
    assert callable(capi.Renderer.overlap_instances) and callable(capi.Renderer.voxel_occupancy_instances)
    assert native_lib.cap_overlap_instances(None, None, 0, 1, None, None, None, 0, None) == ERR_INVALID_ARG
    assert b"cap_overlap_instances: ctx is NULL" in native_lib.cap_last_error()
    assert native_lib.cap_debug_overlap_instance_prune(*([None] * 17)) == ERR_INVALID_ARG


# ---- the reference by hand ----
def test_touching_boxes_under_a_translation_and_a_stretch():
    tris, M, names, boxes, want = touching_instances()
    tab = PairTable(boxes, M, tris)
    assert sum(1 for p in want if not p) >= 14 and sum(1 for n in names if "one ulp" in n) >= 14
    for b, (name, pairs) in enumerate(zip(names, want)):
        got = [(int(tab.inst_of[f]), int(tab.tri_of[f])) for f in tab.candidates(b)]
        assert got == pairs, (name, got, pairs)


def test_a_pair_only_a_cross_axis_of_the_rotated_triangle_separates():
    tris = np.array([[(0, 0, 0), (1, 0, 0), (0, 1, 0)]], f32)
    c = np.sqrt(0.5)
    M = np.stack([identity()[0], affine([[c, -c, 0], [c, c, 0], [0, 0, 1]])])
    box = boxes_of([(0.6, 0.1, -0.1)], [(0.7, 0.2, 0.1)])
    tab = PairTable(box, M, tris)
    assert [int(f) for f in tab.candidates(0)] == [0], "the triangle as uploaded meets the box, its rotated copy does not"
    v0w, e1w, e2w = (x[1] for x in world_records(M, tris))
    by_box, by_cross, by_plane = axes(box[:, 0:3], box[:, 4:7], v0w, e1w, e2w)
    assert not by_box[0, 0] and not by_plane[0, 0] and by_cross[0, 0], "the rotated triangle's vertex box and plane meet the box"


def test_coincident_instances_list_each_triangle_once_per_instance_in_order():
    tris = soup(np.random.default_rng(5), 40, edge=0.3)
    M = np.stack([identity()[0], identity()[0], affine(np.eye(3), (8, 0, 0)), identity()[0]])
    boxes = boxes_near(np.random.default_rng(6), M[:1], tris, 32, away=1000)
    tab, flat = PairTable(boxes, M, tris), Table(boxes, tris)
    for b in range(32):
        ids = flat.candidates(b)
        assert len(ids) > 0 or b == 0  # (box 0 is the one boxes_near moves away)
        want = [(i, int(g)) for i in (0, 1, 3) for g in ids]
        assert [(int(tab.inst_of[f]), int(tab.tri_of[f])) for f in tab.candidates(b)] == want
    # pages: boundaries inside an instance and between the coincident ones, every pair once
    for k in (1, 3, 16):
        walk = pages(tab, k)
        assert all_miss(walk[-1][0]) and all_miss(walk[-1][1]) and not all_miss(walk[-2][0])
        for b in range(32):
            tri = np.concatenate([p[0][b] for p in walk])
            inst = np.concatenate([p[1][b] for p in walk])
            assert ((tri == MISS) == (inst == MISS)).all()
            assert (inst[inst != MISS].astype(np.int64) * 40 + tri[tri != MISS]).tolist() == tab.candidates(b).tolist()
        spans = [len(np.unique(row[row != MISS])) for p in walk for row in p[1]]
        assert max(spans) > 1 or k == 1, "a page spans two instances"
        if k == 3:
            starts = {int(p[1][b, 0]) for p in walk[1:-1] for b in range(32)}
            assert {0, 1, 3} <= starts, "page boundaries inside an instance and between the coincident ones"
        assert (walk[0][2] == tab.counts()).all() and (walk[-1][2] == 0).all()
    assert len(tab.candidates(0, (MISS, MISS))) == 0 and len(tab.candidates(0, (3, 39))) == 0, "the cursor of a short page admits nothing"


def test_inert_masked_instances_and_objects():
    tris = soup(np.random.default_rng(7), 60, edge=0.3)
    M, must_be_inert = extreme_transforms()
    live = live_of(M)
    assert not live[must_be_inert].any() and live.any()
    everything = boxes_of([(-3e38,) * 3], [(3e38,) * 3])
    with np.errstate(all="ignore"):
        tab = PairTable(everything, M, tris)
    valid = pair_valid(len(M), 60, live)
    assert np.array_equal(np.unique(tab.inst_of[tab.with_valid(valid).candidates(0)]), np.nonzero(live)[0])
    im = np.full(len(M), 0xFF, np.uint32)
    im[np.nonzero(live)[0][0]] = 0x02
    masked = tab.with_valid(pair_valid(len(M), 60, live, im, None, 0x01))
    assert np.array_equal(np.unique(masked.inst_of[masked.candidates(0)]), np.nonzero(live)[0][1:])
    mesh = tab.with_valid(pair_valid(len(M), 60, live, None, np.where(np.arange(60) < 30, 0x01, 0x02), 0x02))
    assert (mesh.tri_of[mesh.candidates(0)] >= 30).all() and len(mesh.candidates(0)) == 30 * live.sum()
    obj = tab.with_valid(pair_valid(len(M), 60, live, None, None, None, np.arange(len(M)) % 2, (np.arange(60) >= 20).astype(int)))
    c = obj.candidates(0)
    assert ((obj.tri_of[c] >= 20) == (obj.inst_of[c] % 2 == 1)).all() and len(c) == sum(20 if i % 2 == 0 else 40 for i in np.nonzero(live)[0])


# ---- the three identities ----
def test_one_identity_instance_is_the_flat_query():
    tris = soup_scene()[0][:800]
    flat = Table(soup_table(0.14).b[:128], tris)
    tab = PairTable(flat.b, identity(), tris)
    assert np.array_equal(tab.meets, flat.meets) and flat.meets.any()
    # the sign of a zero is all 1 x + 0 y + 0 z can change
    v0w, e1w, e2w = world_records(identity(), tris)
    for w, o in zip((v0w[0], e1w[0], e2w[0]), records_of(tris)):
        assert np.array_equal(w, o)


def test_translations_on_a_grid_give_the_flattened_scene():
    rng = np.random.default_rng(8)
    _, tris = grid_scene()
    T = rng.integers(-32 * 16, 32 * 16 + 1, (6, 3)) / 16.0
    M = translations(T)
    flat_tris = np.concatenate([(tris.astype(np.float64) + t).astype(f32) for t in T])
    assert np.array_equal(flat_tris.astype(np.float64), np.concatenate([tris.astype(np.float64) + t for t in T])), "every sum is exact"
    c = T[rng.integers(0, 6, 96)] + rng.integers(-8 * 16, 8 * 16 + 1, (96, 3)) / 16.0
    half = rng.integers(0, 4 * 16 + 1, (96, 3)) / 16.0
    boxes = boxes_of((c - half).astype(f32), (c + half).astype(f32))
    tab, flat = PairTable(boxes, M, tris), Table(boxes, flat_tris)
    assert np.array_equal(tab.meets, flat.meets) and 0 < tab.meets.sum() < tab.meets.size
    assert len(np.unique(tab.inst_of[np.nonzero(tab.meets.any(0))[0]])) == 6


def test_scaling_by_a_power_of_two_changes_nothing():
    tris, M, tab = soup_case()
    for j in (-20, 7):
        s = f32(2.0 ** j)
        scaled = meets_pairs((tab.b[:64] * s).astype(f32), (M * s).astype(f32), tris)
        assert np.array_equal(scaled, tab.meets[:64])


# ---- the float64 twin ----
@pytest.mark.parametrize("case", (soup_case, needle_case), ids=("soup", "needles"))
def test_the_reference_agrees_with_its_float64_twin(case):
    tris, M, tab = case()
    twin = meets_pairs(tab.b, M, tris, np.float64)
    differ = int((twin != tab.meets).sum())
    print("%s: %d of %d pairs differ from the float64 twin, %d candidates" % (case.__name__, differ, twin.size, int(tab.meets.sum())))
    assert differ <= 10


# ---- the prune never skips a candidate ----
def candidate_skips(tris, M, tab, live=None):
    """(pairs asked, skipped at the top level, skipped at the node) through the debug entry, for every candidate pair of the table, with
    the triangle's own boxes standing for the boxes above it; the numpy model must say the same"""
    lib = capi.lib()
    olo, ohi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    nlo, nhi, wlo, whi = stand_in_boxes(M, tris)
    asked = top = node = 0
    for i in range(tab.i):
        if live is not None and not live[i]:
            continue
        bs, gs = np.nonzero(tab.meets[:, i * tab.t:(i + 1) * tab.t])
        if len(bs) == 0:
            continue
        first = prune(M[i], olo, ohi, wlo[i, gs[0]], whi[i, gs[0]], nlo[gs[0]], nhi[gs[0]], tab.b[bs[0], 0:3], tab.b[bs[0], 4:7], lib)
        m_top, m_node = model_skips(first["W"], first["g"], first["xw"], wlo[i, gs], whi[i, gs], nlo[gs], nhi[gs], tab.b[bs, 0:3], tab.b[bs, 4:7])
        for n, (b, g) in enumerate(zip(bs, gs)):
            p = prune(M[i], olo, ohi, wlo[i, g], whi[i, g], nlo[g], nhi[g], tab.b[b, 0:3], tab.b[b, 4:7], lib)
            assert (p["skip_top"], p["skip_node"]) == (int(m_top[n]), int(m_node[n])), "the model is the shipped arithmetic"
            top += p["skip_top"]
            node += p["skip_node"]
        asked += len(bs)
    return asked, top, node


@pytest.mark.parametrize("case", (soup_case, far_case, needle_case), ids=("soup", "near 4096", "needles"))
def test_the_prune_skips_no_candidate(native_lib, case):
    tris, M, tab = case()
    asked, top, node = candidate_skips(tris, M, tab)
    print("%s: %d candidate pairs, %d skipped at the top level, %d at the node" % (case.__name__, asked, top, node))
    assert asked > 2000 and top == 0 and node == 0


def test_the_prune_skips_no_candidate_of_extreme_transforms_and_huge_boxes(native_lib):
    tris = soup(np.random.default_rng(42), 120, edge=0.2)
    M, _ = extreme_transforms()
    live = live_of(M)
    boxes = np.concatenate([boxes_near(np.random.default_rng(43), M[live], tris, 64), huge_boxes()])
    with np.errstate(all="ignore"):
        tab = PairTable(boxes, M, tris)
        asked, top, node = candidate_skips(tris, M, tab, live)
    assert tab.with_valid(pair_valid(len(M), 120, live)).counts()[64] == 120 * live.sum(), "the FLT_MAX box lists every live pair"
    assert asked > 120 * live.sum() and top == 0 and node == 0
    # a lopsided huge box under a scaling instance: c' + h' is not finite and opens everything
    S = affine(np.eye(3) * 1e3)
    p = prune(S, (0, 0, 0), (1, 1, 1), (0, 0, 0), (1e3, 1e3, 1e3), (0, 0, 0), (1, 1, 1), (-3.4e38,) * 3, (0, 0, 0))
    assert p["skip_top"] == 0 and p["skip_node"] == 0


def test_without_the_slack_the_prune_loses_candidates_near_4096(native_lib):
    """so that the tests above can fail: the same question of the model with the constant forced to 0"""
    tris, M, tab = far_case()
    olo, ohi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    nlo, nhi, wlo, whi = stand_in_boxes(M, tris)
    lost = kept = 0
    for i in range(tab.i):
        bs, gs = np.nonzero(tab.meets[:, i * tab.t:(i + 1) * tab.t])
        if len(bs) == 0:
            continue
        d = prune(M[i], olo, ohi, wlo[i, gs[0]], whi[i, gs[0]], nlo[gs[0]], nhi[gs[0]], tab.b[bs[0], 0:3], tab.b[bs[0], 4:7])
        for c2, into in ((0.0, "lost"), (C2, "kept")):
            m_top, m_node = model_skips(d["W"], d["g"], d["xw"], wlo[i, gs], whi[i, gs], nlo[gs], nhi[gs], tab.b[bs, 0:3], tab.b[bs, 4:7], c2)
            if into == "lost":
                lost += int((m_top | m_node).sum())
            else:
                kept += int((m_top | m_node).sum())
    print("near 4096 without the slack: %d candidates skipped" % lost)
    assert lost > 0 and kept == 0


def test_the_debug_entry_reports_the_setup_and_the_image(native_lib):
    for M in regular_transforms(12):
        p = prune(M, (0, 0, 0), (1, 1, 1), (0, 0, 0), (1, 1, 1), (0, 0, 0), (1, 1, 1), (-1, -2, -3), (4, 5, 6))
        L = M[:, :3].astype(np.float64)
        assert 0 < p["g"] <= np.linalg.svd(L, compute_uv=False)[-1] and p["g"] > 0.999 * np.linalg.svd(L, compute_uv=False)[-1]
        assert np.allclose(p["W"][:, :3].astype(np.float64) @ L, np.eye(3), atol=1e-4)
        assert p["xw"] >= np.abs(M[:, 3]).max() and np.float32(p["slack"]) == (C2 * f32(2.0 ** -24)) * (f32(6.0) + f32(p["xw"]))
        slack, olo, ohi = model_image(p["W"], p["g"], p["xw"], f32([-1, -2, -3]), f32([4, 5, 6]))
        assert np.array_equal(olo, p["image_lo"]) and np.array_equal(ohi, p["image_hi"]) and f32(p["slack"]) == slack
        # the image holds the exact images of the box's corners
        W = p["W"].astype(np.float64)
        corners = np.array([[(4, 5, 6)[k] if (c >> k) & 1 else (-1, -2, -3)[k] for k in range(3)] for c in range(8)], np.float64)
        q = corners @ W[:, :3].T + W[:, 3]
        assert (q >= olo).all() and (q <= ohi).all()
    inert = prune(np.zeros((3, 4), f32), (0, 0, 0), (1, 1, 1), (5, 5, 5), (6, 6, 6), (5, 5, 5), (6, 6, 6), (0, 0, 0), (1, 1, 1))
    assert inert["g"] == 0 and inert["xw"] == 0 and inert["skip_top"] == 0 and inert["skip_node"] == 0 and not inert["W"].any()
    far = prune(identity()[0], (0, 0, 0), (1, 1, 1), (5, 5, 5), (6, 6, 6), (5, 5, 5), (6, 6, 6), (0, 0, 0), (1, 1, 1))
    assert far["skip_top"] == 1 and far["skip_node"] == 1
    touch = prune(identity()[0], (0, 0, 0), (1, 1, 1), (1, 1, 1), (6, 6, 6), (1, 1, 1), (6, 6, 6), (0, 0, 0), (1, 1, 1))
    assert touch["skip_top"] == 0 and touch["skip_node"] == 0


# ---- the address checks of the call's four arrays ----
BASE = 1 << 40


def layout_of(k):
    """boxes, triangle pages, instance pages, counts: (bytes per box, alignment); stride 0 = left out (k = 0)"""
    return ((32, 16), (4 * k, 4), (4 * k, 4), (4, 4))


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
    table.append(("2^62 boxes", 1 << 62, apart, ERR_INVALID_ARG, ("address space",)))
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
    assert min(classes) >= 8, "boxes with 0, 1..k, k+1..3k and more pairs: %s" % classes
    _, inst, _ = tab.page(k)
    assert len(np.unique(inst[inst != MISS])) >= 16, "pairs of many instances in the pages"


def test_pages_of_the_soup_span_instances():
    _, _, tab = soup_case()
    _, inst, _ = tab.page(16)
    spans = sum(1 for row in inst if len(np.unique(row[row != MISS])) > 1)
    assert spans >= 16, "boxes that meet several instances (the coincident ones of regular_transforms)"
    assert len(cursors_of(*tab.page(3)[:2])) == tab.n
