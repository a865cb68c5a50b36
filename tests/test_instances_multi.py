"""Multi-hit instanced ray queries (cap_trace_instances_multi) without a GPU: the header's prototype, the export and the binding, the
NULL context, and the page / cursor helpers of the GPU tests on a hand-written hit list."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi
from instance_multi_support import MISS, START, above, bits, cursor_of, expected_pages, f32, key, listed, next_page, page, walk, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_prototype_compiles(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "instances_multi.c"
    src.write_text("""#include "capsaicin_hip.h"
_Static_assert(CAP_MULTI_MAX_K == 16 && CAP_MULTI_CONTINUE == 1, "the multi-hit constants are cap_trace_rays_multi's");
int (*const multi)(CapContext*, const CapRayDesc*, uint64_t, uint32_t, CapHit*, uint32_t*, uint32_t*, uint32_t, const CapTraceOptions*) =
    cap_trace_instances_multi;
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "instances_multi.o")])


def test_entry_point_is_exported_and_bound(native_lib):
    assert hasattr(native_lib, "cap_trace_instances_multi")
    assert "cap_trace_instances_multi" in capi.SYMBOLS
    assert len(capi.SYMBOLS["cap_trace_instances_multi"][1]) == 9
    assert callable(capi.Renderer.trace_instances_multi)


def test_null_context_is_rejected_by_name(native_lib):
    assert native_lib.cap_trace_instances_multi(None, None, 0, 1, None, None, None, 0, None) != 0
    assert b"cap_trace_instances_multi: ctx is NULL" in native_lib.cap_last_error()


# t = 1 three times: twice the same triangle in two instances, twice the same instance with two triangles
HITS = [(f32(0.5), f32(0.25), f32(0.5), 3, 7), (f32(1), f32(0), f32(1), 1, 4), (f32(1), f32(0.5), f32(0.5), 2, 4), (f32(1), f32(0.125), f32(0.25), 2, 9),
        (f32(2), f32(0), f32(0), 0, 0), (f32(2.5), f32(0.75), f32(0.125), 0, 11), (f32(4), f32(0.5), f32(0.25), 5, 1)]
TMAX = f32(8)


def test_hit_list_is_in_contract_order():
    assert [key(h) for h in HITS] == sorted(key(h) for h in HITS) and len({key(h) for h in HITS}) == len(HITS)
    assert above(HITS, START) == HITS and above(HITS, (1.0, 2, 4)) == HITS[3:] and above(HITS, (1.0, 1, 0xFFFFFFFF)) == HITS[2:]
    assert above(HITS, (float(TMAX), MISS, MISS)) == [], "the miss record's cursor admits nothing"


@pytest.mark.parametrize("k", (1, 2, 3))
def test_pages_reproduce_the_list_exactly_once(k):
    calls = walk(HITS, k, TMAX)
    assert len(calls) == -(-len(HITS) // k) + 1, "the pages that hold something, then one empty one"
    got = []
    for n, (rec, inst, count) in enumerate(calls):
        assert rec.shape == (k, 4) and inst.shape == (k,) and rec.dtype == np.uint32
        assert count == max(len(HITS) - n * k, 0), "counts are the pairs above the cursor, not capped at k"
        got += listed(rec, inst)
    assert got == words(HITS), "every pair exactly once, in order"
    # the walk ends in miss records: the last call is empty, and a short page is padded with them
    rec, inst, count = calls[-1]
    miss = np.array([bits(TMAX)[0], 0, 0, MISS], np.uint32)
    assert count == 0 and np.all(rec == miss) and np.all(inst == MISS)
    if len(HITS) % k:
        rec, inst, _ = calls[-2]
        assert np.all(rec[len(HITS) % k:] == miss) and np.all(inst[len(HITS) % k:] == MISS)
        assert cursor_of(rec, inst) == (float(TMAX), MISS, MISS)
    # the equal-t pairs straddle page boundaries at k = 1 and k = 3 and are kept
    flat = [x[3:] for x in got]
    assert flat.index((1, 4)) + 1 == flat.index((2, 4)) and flat.index((2, 4)) + 1 == flat.index((2, 9))


@pytest.mark.parametrize("k", (1, 2, 3))
def test_positions_and_cursors_agree(k):
    """the GPU tests page by position in the list; that is the cursor rule because the list is strictly ascending"""
    rays = np.zeros((1, 8), f32)
    rays[0, 7] = TMAX
    cursor = START
    for start in range(0, len(HITS) + k, k):
        rec, inst, cnt = expected_pages([HITS], rays, k, start)
        a, b, c = next_page(HITS, k, TMAX, cursor)
        assert np.array_equal(rec[0], a) and np.array_equal(inst[0], b) and cnt[0] == c
        cursor = cursor_of(a, b)


def test_page_of_nothing_and_of_zero_slots():
    rec, inst = page([], 2, f32(np.inf))
    assert rec.tolist() == [[0x7F800000, 0, 0, MISS]] * 2 and inst.tolist() == [MISS, MISS]
    rec, inst, count = next_page(HITS, 0, TMAX)
    assert rec.shape == (0, 4) and inst.shape == (0,) and count == len(HITS), "k = 0 counts only"
