"""k-nearest / in-radius closest-point queries over instances (cap_closest_instances_multi) without a GPU: the header's prototype, the
export and the binding, the brute force of closest_instances_multi_support.py against closest_instances_support's single answer, against
closest_multi_support's flat table and against itself, and the address checks of the call's four arrays."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_instances_multi_support import PairTable, all_miss, assert_counts, assert_pair_pages, cursors_of, listed, pages, tie_case
from closest_instances_support import assert_pairs, closest_instances, identity, pair_valid, world_hull_points, world_points_near
from closest_multi_support import Table, assert_pages
from closest_point_support import MISS, around, bits, queries, soup
from instance_support import regular_transforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID_ARG = 0, 1


def test_header_prototype_compiles(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "closest_instances_multi.c"
    src.write_text("""#include "capsaicin_hip.h"
_Static_assert(CAP_MULTI_MAX_K == 16 && CAP_MULTI_CONTINUE == 1, "the multi-hit queries' page limit and flag");
int (*const closest_instances_multi)(CapContext*, const CapPointDesc*, uint64_t, uint32_t, CapClosest*, uint32_t*, uint32_t*, uint32_t,
                                     const CapTraceOptions*) = cap_closest_instances_multi;
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "closest_instances_multi.o")])


def test_entry_point_is_exported_and_bound(native_lib):
    assert hasattr(native_lib, "cap_closest_instances_multi")
    assert len(capi.SYMBOLS["cap_closest_instances_multi"][1]) == 9
    assert callable(capi.Renderer.closest_instances_multi)
    assert native_lib.cap_closest_instances_multi(None, None, 0, 1, None, None, None, 0, None) == ERR_INVALID_ARG
    assert b"cap_closest_instances_multi: ctx is NULL" in native_lib.cap_last_error()


# ---- the brute force against the single answer ----
def test_the_first_slot_is_the_single_answer():
    rng = np.random.default_rng(31)
    tris = soup(rng, 150, edge=0.2)
    M = regular_transforms(8)
    q = queries(np.concatenate([world_hull_points(rng, M, tris, 60, 0.05), world_points_near(rng, M, tris, 60, 0.02)]))
    free = closest_instances(q[60:], M, tris)
    q[60:, 3] = np.sqrt(free[0][:, 3]) * rng.uniform(0.5, 1.5, 60).astype(np.float32)
    q[3, 0], q[5, 3], q[70, 3] = np.nan, -1.0, np.nan
    imasks = np.uint32([0x01, 0x02, 0x04, 0xFF, 0x03, 0x00, 0x01, 0x02])
    tm = np.where(np.arange(150) < 75, 0x05, 0x02).astype(np.uint32)
    for valid in (None, pair_valid(8, 150, None, imasks, tm, 0x07)):
        want = closest_instances(q, M, tris, valid)
        tab = PairTable(q, M, tris, valid)
        rec, inst, cnt = tab.page(1)
        hit = want[1] >= 0
        assert 10 < hit[60:].sum() < 55 and hit[:60].sum() == 58
        assert_pairs((rec[:, 0], inst[:, 0]), want, "k = 1")
        assert ((cnt > 0) == hit).all()
        rec5, inst5, _ = tab.page(5)
        assert_pairs((rec5[:, 0], inst5[:, 0]), want, "slot 0 of k = 5")


# ---- the brute force against itself ----
def test_pages_walk_every_pair_once():
    tris, M, q = tie_case()
    tab = PairTable(q, M, tris)
    T = len(tris)
    full = [tab.candidates(i) for i in range(tab.n)]
    sizes = [len(f) for f in full]
    distinct = [len(np.unique(tab.d2[i, f])) for i, f in enumerate(full)]
    assert min(sizes) >= 16 and max(sizes) <= 24 and max(distinct) <= 3, (sizes, distinct)
    for i, f in enumerate(full):  # sorted by (dist2, instance, triangle), every pair once, runs that span instances
        key = list(zip(tab.d2[i, f].tolist(), (f // T).tolist(), (f % T).tolist()))
        assert key == sorted(key) and len(set(f.tolist())) == len(f)
        first_run = f[tab.d2[i, f] == tab.d2[i, f[0]]]
        assert len(np.unique(first_run // T)) >= 3
    assert_counts(tab.counts(), sizes)
    for k in (1, 2, 3, 5, 16):
        walk = pages(tab, k)
        assert all_miss(walk[-1][0]) and not all_miss(walk[-2][0])
        seen = np.zeros(tab.n, np.int64)
        for rec, inst, cnt in walk:
            assert_counts(cnt, np.array(sizes) - seen, "the remainder, k = %d" % k)
            seen += (bits(rec)[..., 6] != MISS).sum(1)
        for i, f in enumerate(full):
            rows, inst = listed(walk, i)
            assert (inst.astype(np.int64) * T + bits(rows)[:, 6]).tolist() == f.tolist(), (k, i)
            assert_pair_pages((rows, inst), (tab.records(i, f), f // T), "k = %d point %d" % (k, i))


def test_a_miss_records_cursor_admits_nothing():
    tris, M, q = tie_case()
    q[::2, 3] = 0.0625  # r2 = dist2 of the nearest plane's triangles: pairs AT the limit
    tab = PairTable(q, M, tris)
    rec, inst, cnt = tab.page(16)
    at_limit = [(tab.d2[i, tab.candidates(i)] == tab.r2[i]).sum() for i in range(0, tab.n, 2)]
    assert min(at_limit) >= 2 and (cnt[::2] < 16).all() and (cnt[::2] > 0).all()
    again, inst2, cnt2 = tab.page(16, cursors_of(rec, inst))
    short = cnt < 16
    assert short.sum() >= tab.n // 2 and all_miss(again[short]) and (inst2[short] == -1).all() and (cnt2[short] == 0).all()
    assert cursors_of(rec[short], inst[short])[0] == (float(tab.r2[np.nonzero(short)[0][0]]), MISS, MISS)
    for k in (1, 3):  # ... and a walk ends with them listed once
        walk = pages(tab, k)
        for i in range(0, tab.n, 2):
            rows, li = listed(walk, i)
            assert (li.astype(np.int64) * len(tris) + bits(rows)[:, 6]).tolist() == tab.candidates(i).tolist()


def test_inert_and_masked_instances_never_appear():
    rng = np.random.default_rng(32)
    tris = soup(rng, 100, edge=0.2)
    M = regular_transforms(6)
    q = queries(world_hull_points(rng, M, tris, 40, 0.05))
    live = np.array([True, False, True, True, False, True])
    imasks = np.uint32([0xFF, 0xFF, 0x02, 0x01, 0xFF, 0x00])
    tab = PairTable(q, M, tris, pair_valid(6, 100, live, imasks, None, 0x01))
    rec, inst, cnt = tab.page(16)
    assert set(np.unique(inst).tolist()) == {0, 3} and (cnt == 200).all()
    everything = PairTable(q, M, tris)
    assert (everything.counts() == 600).all()


def test_one_identity_instance_is_the_flat_table():
    rng = np.random.default_rng(33)
    tris = soup(rng, 200, edge=0.15)
    q = queries(around(rng, tris, 64, 0.3))
    q[32:, 3] = rng.random(32).astype(np.float32) * 0.3
    q[7, 1] = np.inf
    flat, inst = Table(q, tris), PairTable(q, identity(), tris)
    for k in (1, 4, 16):
        want, want_cnt = flat.page(k)
        rec, li, cnt = inst.page(k)
        assert_pages(rec, want, "k = %d" % k)
        assert_counts(cnt, want_cnt)
        assert ((li == 0) == (bits(want)[..., 6] != MISS)).all() and ((li == 0) | (li == -1)).all()


def test_degenerate_points_have_no_pairs():
    tris, M, q = tie_case()
    q = q[:6].copy()
    q[0, 0], q[1, 1], q[2, 3], q[3, 3] = np.nan, np.inf, -1.0, np.nan
    tab = PairTable(q, M, tris)
    rec, inst, cnt = tab.page(3)
    want = np.zeros(8, np.uint32)
    want[6] = MISS
    assert (bits(rec[:4]) == want).all() and (inst[:4] == -1).all() and (cnt[:4] == 0).all() and (cnt[4:] > 3).all()
    again, inst2, cnt2 = tab.page(3, cursors_of(rec, inst))
    assert (bits(again[:4]) == want).all() and (inst2[:4] == -1).all() and (cnt2[:4] == 0).all()


# ---- the address checks of the call's four arrays ----
BASE = 1 << 40


def layout_of(k):
    """points, record pages, instance pages, counts: (bytes per point, alignment); stride 0 = left out (k = 0)"""
    return ((16, 16), (32 * k, 16), (4 * k, 4), (4, 4))


def range_cases(layout):
    n = 1000
    size = [n * s for s, _ in layout]
    apart = [BASE + (i << 30) for i in range(4)]
    out = [("apart", n, apart, OK, ())]
    for i, (s, a) in enumerate(layout):
        if not s:
            continue
        b = list(apart)
        b[i] += a // 2
        out.append(("range %d misaligned" % i, n, b, ERR_INVALID_ARG, ("range %d" % i, "aligned")))
    for i in range(4):
        for j in range(4):
            if i == j or not layout[i][0] or not layout[j][0]:
                continue
            b = list(apart)
            b[j] = b[i] + size[i]
            out.append(("range %d right behind range %d" % (j, i), n, b, OK, ()))
            b = list(apart)
            b[j] = b[i] + size[i] - layout[j][1]
            out.append(("range %d starts in the last bytes of range %d" % (j, i), n, b, ERR_INVALID_ARG, ("overlap",)))
    out.append(("2^62 records", 1 << 62, apart, ERR_INVALID_ARG, ("address space",)))
    return out


@pytest.mark.parametrize("k", (1, 16, 0))
def test_query_ranges_of_the_call(native_lib, k):
    """the call's arrays are CapPointDesc (16 B), k CapClosest (32 k B), k uint32 (4 k B) and a uint32 count (4 B) per point; with k = 0
    the record and instance arrays are left out and never looked at, wherever they point"""
    layout = layout_of(k)
    strides, aligns = (C.c_uint64 * 4)(*[s for s, _ in layout]), (C.c_uint32 * 4)(*[a for _, a in layout])
    table = range_cases(layout)
    assert len(table) >= (30 if k else 8)
    for label, n, bases, code, words in table:
        if k == 0:
            bases = [bases[0], bases[0], bases[3], bases[3]]
        assert native_lib.cap_debug_query_ranges(n, 4, (C.c_uint64 * 4)(*bases), strides, aligns) == code, (label, native_lib.cap_last_error())
        message = native_lib.cap_last_error().decode()
        if code:
            assert all(w in message for w in words), (label, message)
