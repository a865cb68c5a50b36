"""k-nearest / in-radius closest-point queries (cap_closest_points_multi) without a GPU: the header's prototype, the export and the
binding, and the brute force of closest_multi_support.py against closest_point_support's single answer and against itself."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_multi_support import Table, all_miss, assert_counts, assert_pages, cursors_of, listed, pages
from closest_point_support import MISS, around, bits, closest, queries, soup
from multi_hit_support import stacked_quads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = 1


def test_header_prototype_compiles(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "closest_multi.c"
    src.write_text("""#include "capsaicin_hip.h"
_Static_assert(CAP_MULTI_MAX_K == 16 && CAP_MULTI_CONTINUE == 1, "the multi-hit queries' page limit and flag");
int (*const closest_multi)(CapContext*, const CapPointDesc*, uint64_t, uint32_t, CapClosest*, uint32_t*, uint32_t, const CapTraceOptions*) =
    cap_closest_points_multi;
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "closest_multi.o")])


def test_entry_point_is_exported_and_bound(native_lib):
    assert hasattr(native_lib, "cap_closest_points_multi")
    assert len(capi.SYMBOLS["cap_closest_points_multi"][1]) == 8
    assert callable(capi.Renderer.closest_points_multi)
    assert native_lib.cap_closest_points_multi(None, None, 0, 1, None, None, 0, None) == ERR_INVALID_ARG
    assert b"cap_closest_points_multi: ctx is NULL" in native_lib.cap_last_error()


def test_closest_triangles_reads_pages():
    page = np.zeros((2, 3, 8), np.float32)
    page.view(np.uint32)[..., 6] = [[7, 9, MISS], [1 << 31, MISS, MISS]]
    page.view(np.uint32)[..., 7] = [[6, 1, 0], [3, 0, 0]]
    ids, feat = capi.closest_triangles(page)
    assert ids.tolist() == [[7, 9, MISS], [1 << 31, MISS, MISS]] and feat.tolist() == [[6, 1, 0], [3, 0, 0]]
    import torch
    ids_t, feat_t = capi.closest_triangles(torch.from_numpy(page))
    assert ids_t.tolist() == ids.tolist() and feat_t.tolist() == feat.tolist()


# ---- the brute force agrees with itself ----
def test_the_first_slot_is_the_single_answer():
    rng = np.random.default_rng(7)
    tris = soup(rng, 600, edge=0.1)
    q = queries(around(rng, tris, 200, 0.3))
    q[100:, 3] = rng.random(100).astype(np.float32) * 0.3
    q[3, 0], q[5, 3], q[150, 3] = np.nan, -1.0, np.nan
    mask = rng.random(len(tris)) < 0.7
    for m in (None, mask):
        want, _ = closest(q, tris, m)
        tab = Table(q, tris, m)
        page, cnt = tab.page(1)
        hit = bits(want)[:, 6] != MISS
        assert 15 < hit[100:].sum() < 95 and hit[:100].sum() == 98
        assert_pages(page[:, 0], want, "k = 1")
        assert ((cnt > 0) == hit).all()
        assert_pages(tab.page(5)[0][:, 0], want, "slot 0 of k = 5")


def tie_case():
    _, tris = stacked_quads(40, 0.25)
    tris = np.concatenate([tris, tris])
    z = (np.arange(39) + 0.5) * 0.25
    pts = [(0.5, 0.5, zz) for zz in z[::4]] + [(0.25, 0.25, zz) for zz in z[1::4]] + [(0.75, 0.75, zz) for zz in z[2::4]]
    return tris, queries(pts, 0.8)


def test_pages_walk_every_candidate_once():
    tris, q = tie_case()
    tab = Table(q, tris)
    full = [tab.candidates(i) for i in range(tab.n)]
    sizes = [len(f) for f in full]
    distinct = [len(np.unique(tab.d2[i, f])) for i, f in enumerate(full)]
    assert min(sizes) >= 16 and max(sizes) <= 24 and max(distinct) <= 3, (sizes, distinct)
    for i, f in enumerate(full):  # sorted by (dist2, id), every triangle once
        key = list(zip(tab.d2[i, f].tolist(), f.tolist()))
        assert key == sorted(key) and len(set(f.tolist())) == len(f)
    assert_counts(tab.counts(), sizes)
    for k in (1, 2, 3, 5, 16):
        walk = pages(tab, k)
        assert all_miss(walk[-1][0]) and not all_miss(walk[-2][0])
        seen = np.zeros(tab.n, np.int64)
        for page, cnt in walk:
            assert_counts(cnt, np.array(sizes) - seen, "the remainder, k = %d" % k)
            seen += (bits(page)[..., 6] != MISS).sum(1)
        for i, f in enumerate(full):
            rows = listed([p for p, _ in walk], i)
            assert bits(rows)[:, 6].tolist() == f.tolist(), (k, i)
            assert_pages(rows, np.stack([tab.record(i, g) for g in f]), "k = %d point %d" % (k, i))


def test_a_miss_records_cursor_admits_nothing():
    tris, q = tie_case()
    q[::2, 3] = 0.125  # r2 = dist2 of the nearest planes' triangles: candidates AT the limit
    tab = Table(q, tris)
    page, cnt = tab.page(16)
    at_limit = [(tab.d2[i, tab.candidates(i)] == tab.r2[i]).sum() for i in range(0, tab.n, 2)]
    assert min(at_limit) >= 2 and (cnt[::2] < 16).all() and (cnt[::2] > 0).all()
    again, cnt2 = tab.page(16, cursors_of(page))
    short = cnt < 16
    assert short.sum() >= tab.n // 2 and all_miss(again[short]) and (cnt2[short] == 0).all()
    assert cursors_of(page[short])[0] == (float(tab.r2[np.nonzero(short)[0][0]]), MISS)
    for k in (1, 3):  # ... and a walk ends with them listed once
        walk = pages(tab, k)
        for i in range(0, tab.n, 2):
            assert bits(listed([p for p, _ in walk], i))[:, 6].tolist() == tab.candidates(i).tolist()


def test_degenerate_queries_have_no_candidates():
    tris, q = tie_case()
    q = q[:6].copy()
    q[0, 0], q[1, 1], q[2, 3], q[3, 3] = np.nan, np.inf, -1.0, np.nan
    tab = Table(q, tris)
    page, cnt = tab.page(3)
    want = np.zeros(8, np.uint32)
    want[6] = MISS
    assert (bits(page[:4]) == want).all() and (cnt[:4] == 0).all() and (cnt[4:] > 3).all()
    again, cnt2 = tab.page(3, cursors_of(page))
    assert (bits(again[:4]) == want).all() and (cnt2[:4] == 0).all()
