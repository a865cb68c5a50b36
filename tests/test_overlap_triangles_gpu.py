"""Triangle overlap queries on the GPU (cap_overlap_triangles): every id of every page and every count compared bit for bit with the numpy
float32 brute force of overlap_triangles_support.py over every triangle, and on the lattice with the exact integer test.
tests/test_overlap_triangles.py asserts without a GPU that the cases below reach what they are named after."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import arrays, context
from overlap_support import boxes_of
from overlap_triangles_support import (MISS, NONE, TriTable, all_miss, assert_counts, assert_pages, contact_case, cursors_of, far_case, fill_scale, ids_of, lattice_case,
                                       needle_case, queries_of_tris, skips_of, soup_scene, soup_table, tris_around, vertices_of)

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 3
CONTINUE = capi.Renderer.MULTI_CONTINUE
CANARY = 0x7FC0BEEF
B = capi.Renderer  # the CapBvhBuild values


def check(r, tab, k, what, counts="both", mask=None):
    """the first page of the table's queries, with and / or without counts, against the brute force"""
    want, cnt = tab.page(k)
    for c in ((False, True) if counts == "both" else (counts,)):
        if c:
            page, got = r.overlap_triangles(tab.b, k, counts=True, mask=mask)
            assert_counts(got, cnt, "%s, k = %d: counts" % (what, k))
        else:
            page = r.overlap_triangles(tab.b, k, mask=mask)
        assert page.shape == (tab.n, k) and page.dtype == np.int32
        assert_pages(page, want, "%s, k = %d%s" % (what, k, ", counts" if c else ""))


class Raw:
    """the C call on torch buffers filled with canaries: `pad` queries' worth of them behind the page and the counts"""

    def __init__(self, r, queries, k, pad=4, counts=True):
        import torch
        self.r, self.n, self.k, self.L = r, len(queries), k, capi.lib()
        dev = torch.device("cuda", 0)
        self.queries = torch.as_tensor(np.ascontiguousarray(queries, np.float32), device=dev).contiguous()
        self.page = torch.full(((self.n + pad) * max(k, 1),), CANARY, dtype=torch.int32, device=dev)
        self.cnt = torch.full((self.n + pad,), CANARY, dtype=torch.int32, device=dev) if counts else None
        torch.cuda.synchronize()

    def call(self, flags=0, options=None):
        rc = self.L.cap_overlap_triangles(self.r.ctx, self.queries.data_ptr(), self.n, self.k, self.page.data_ptr() if self.k else None,
                                          self.cnt.data_ptr() if self.cnt is not None else None, flags, options)
        self.r.sync()
        return rc

    def read(self):
        """(page (n, k) uint32, counts (n,) or None); asserts the canaries behind both"""
        words = self.page.cpu().numpy().view(np.uint32)
        head = self.n * self.k
        assert (words[head:] == CANARY).all(), "nothing behind the last id"
        cnt = None
        if self.cnt is not None:
            c = self.cnt.cpu().numpy().view(np.uint32)
            assert (c[self.n:] == CANARY).all(), "nothing behind the last count"
            cnt = c[:self.n]
        return words[:head].reshape(self.n, self.k), cnt

    def untouched(self):
        return bool((self.page == CANARY).all()) and (self.cnt is None or bool((self.cnt == CANARY).all()))


@pytest.fixture(scope="module")
def soup_ctx(native_lib):
    r = context([soup_scene()[0]])
    yield r
    r.close()


# 1. both sides of every K bucket; empty, part-filled, just-filled and overfull pages
@pytest.mark.parametrize("k", (1, 2, 4, 5, 8, 9, 16))
def test_buckets_and_page_fill(soup_ctx, k):
    check(soup_ctx, soup_table(fill_scale(k)), k, "soup")


def test_counts_only(soup_ctx):
    tab = soup_table(0.8)
    page, got = soup_ctx.overlap_triangles(tab.b, 0, counts=True)
    assert page.shape == (tab.n, 0)
    assert_counts(got, tab.counts(), "k = 0")


# 2. paging
@pytest.mark.parametrize("k", (1, 3, 16))
def test_pages_to_exhaustion(soup_ctx, k):
    tab = soup_table(0.8).first(64 if k == 1 else 256)
    full = [tab.candidates(i) for i in range(tab.n)]
    sizes = np.array([len(f) for f in full])
    assert 16 < sizes.max() <= 110 and (sizes == 0).any()
    got_pages, seen, page = [], np.zeros(tab.n, np.int64), None
    for _ in range(sizes.max() // k + 2):
        page, cnt = soup_ctx.overlap_triangles(tab.b, k, counts=True, resume=page)
        assert_counts(cnt, sizes - seen, "the remainder before page %d, k = %d" % (len(got_pages), k))
        got_pages.append(ids_of(page).copy())
        seen += (got_pages[-1] != MISS).sum(1)
        if all_miss(page):
            break
    assert all_miss(got_pages[-1]) and len(got_pages) == -(-int(sizes.max()) // k) + 1, "the page after a short or a just-full page is empty"
    for i, f in enumerate(full):
        rows = np.concatenate([p[i] for p in got_pages])
        assert rows[rows != MISS].tolist() == f.tolist(), "k = %d query %d: every candidate once, in id order" % (k, i)
    # the same walk without counts gives the same pages
    page = None
    for n, want in enumerate(got_pages):
        page = soup_ctx.overlap_triangles(tab.b, k, resume=page)
        assert_pages(page, want, "k = %d page %d without counts" % (k, n))


# 3. the lattice: the kernel against the truth
def test_lattice_equals_the_exact_integer_test_and_lies_within_the_box_query(native_lib):
    scene, queries, exact = lattice_case()
    tris = scene.astype(np.float32)
    q = queries_of_tris(queries)
    tab = TriTable(q, tris)
    assert np.array_equal(tab.meets, exact), "the transcription is the exact test on the lattice"
    A = vertices_of(q)
    boxes = boxes_of(A.min(1), A.max(1))  # (integer corners: the box query's centred frame is exact on half-integers)
    r = context([tris])
    try:
        _, cnt = r.overlap_triangles(q, 0, counts=True)
        assert_counts(cnt, exact.sum(1), "lattice counts against the exact test")
        _, box_cnt = r.overlap_boxes(boxes, 0, counts=True)
        assert (np.asarray(box_cnt) >= np.asarray(cnt)).all()
        want = np.full((len(q), 16), MISS, np.uint32)
        for i in range(len(q)):
            ids = np.nonzero(exact[i])[0][:16]
            want[i, :len(ids)] = ids
        page, box_page = None, None
        listed = [[] for _ in q]
        in_box = [[] for _ in q]
        for n in range(-(-len(tris) // 16) + 1):
            page = r.overlap_triangles(q, 16, resume=page)
            if n == 0:
                assert_pages(page, want, "lattice, the first page against the exact test")
            box_page = r.overlap_boxes(boxes, 16, resume=box_page)
            for i in range(len(q)):
                listed[i] += [g for g in ids_of(page)[i].tolist() if g != MISS]
                in_box[i] += [g for g in ids_of(box_page)[i].tolist() if g != MISS]
            if all_miss(page) and all_miss(box_page):
                break
        for i in range(len(q)):
            assert listed[i] == np.nonzero(exact[i])[0].tolist(), "query %d: all pages against the exact test" % i
            assert set(listed[i]) <= set(in_box[i]), "query %d: every candidate is a candidate of its bounding box" % i
        assert sum(len(b) for b in in_box) > sum(len(x) for x in listed)
    finally:
        r.close()


# 4. crafted scenes
@pytest.mark.parametrize("twice", (False, True), ids=("once", "twice"))
def test_contacts_on_the_stacked_quads(native_lib, twice):
    tris, names, queries, want = contact_case(twice)
    tab = TriTable(queries, tris)
    r = context([tris])
    try:
        page, cnt = r.overlap_triangles(queries, 16, counts=True)
        for i, (name, ids) in enumerate(zip(names, want)):
            got = ids_of(page)[i]
            assert got[got != MISS].tolist() == ids[:16] and cnt[i] == len(ids), name
        for k in (1, 4, 16):
            check(r, tab, k, "stacked quads")
    finally:
        r.close()


def test_skip_through_scene_triangle_queries(native_lib):
    """a triangle's self query lists its neighbours and not itself; with skip at 0xFFFFFFFF it lists itself; an id beyond the scene
    skips nothing"""
    tris, _, _, _ = contact_case()
    r = context([tris[:6], tris[6:]])  # (two meshes: the ids run through both)
    try:
        ids = np.arange(len(tris))
        q = r.scene_triangle_queries(ids)
        assert q.shape == (16, 12) and q.dtype == np.float32 and skips_of(q).tolist() == ids.tolist()
        assert np.array_equal(vertices_of(q), tris), "the uploaded vertices"
        page, cnt = r.overlap_triangles(q, 4, counts=True)
        for g in ids:
            assert ids_of(page)[g].tolist() == [g ^ 1, MISS, MISS, MISS] and cnt[g] == 1, "triangle %d touches the other half of its quad alone" % g
        check(r, TriTable(q, tris), 4, "self queries")
        free = q.copy()
        free.view(np.uint32)[:, 3] = NONE
        page, cnt = r.overlap_triangles(free, 4, counts=True)
        for g in ids:
            assert ids_of(page)[g].tolist() == sorted([g, g ^ 1]) + [MISS, MISS] and cnt[g] == 2
        beyond = q.copy()
        beyond.view(np.uint32)[:, 3] = np.where(ids % 2 == 0, len(tris), 0x7FFFFFFF).astype(np.uint32)
        assert_pages(r.overlap_triangles(beyond, 4), page, "an out-of-range skip changes nothing")
        # the next page under skip, and skip under a mask
        tab = TriTable(r.scene_triangle_queries([4, 5, 9]), tris)
        one = r.overlap_triangles(tab.b, 1)
        assert_pages(one, tab.page(1)[0], "self queries, k = 1")
        assert all_miss(r.overlap_triangles(tab.b, 1, resume=one))
        # after an update the rows are the new vertices
        P = arrays(tris[:6], tris[6:])[0]
        moved = (P + np.float32([0.5, 0.25, 0.125])).astype(np.float32)
        r.update_vertices(positions=moved)
        r.refit_bvh()
        assert np.array_equal(vertices_of(r.scene_triangle_queries(ids)), moved.reshape(-1, 3, 3))
        with pytest.raises(capi.CapError):
            r.scene_triangle_queries([16])
    finally:
        r.close()


@pytest.mark.parametrize("case", (far_case, needle_case), ids=("near 4096", "needles"))
def test_far_coordinates_and_needles(native_lib, case):
    tris, tab = case()
    r = context([tris])
    try:
        for k in (4, 16):
            check(r, tab, k, case.__name__)
    finally:
        r.close()


def test_far_and_non_finite_queries_in_one_batch(soup_ctx):
    tris = soup_scene()[0]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    A = vertices_of(soup_table(1.5).b[:96]).copy()
    A[1::12] = [(-3, -3, 0.5), (5, -3, 0.5), (1, 6, 0.5)]                   # a plane through the whole scene
    A[2::12] = [(1e6, 1e6, 1e6), (2e6, 1e6, 1e6), (1e6, 2e6, 2e6)]          # far outside the scene
    A[3::12] = [(-1e30, 0.5, 0.5), (-1e30, 1, 0.5), (-1e29, 0.5, 1)]
    A[4::12] = [(-1e18, 0.25, 0.5), (1e18, 0.75, 0.5), (1e18, 0.75, 0.5)]   # a segment through the scene from far away
    A[5::12, 0, 0] = nan
    A[6::12, 1, 1] = inf
    A[7::12, 2, 2] = -inf
    A[8::12, 1, 0] = nan
    A[9::12, 2, 1] = nan
    A[10::12] = nan
    q = queries_of_tris(A)
    tab = TriTable(q, tris)
    cnt = tab.counts()
    assert tab.bad.sum() == 48 and (cnt[1::12] > 50).all() and (cnt[2::12] == 0).all() and (cnt[3::12] == 0).all()
    assert (cnt[0::12] > 0).sum() >= 4
    for k in (3, 16):
        want, _ = tab.page(k)
        assert (want[tab.bad] == MISS).all()
        for counts in (True, False):
            raw = Raw(soup_ctx, q, k, counts=counts)
            assert raw.call() == 0
            page, got = raw.read()
            assert_pages(page, want, "mixed batch, k = %d" % k)
            if counts:
                assert_counts(got, cnt, "mixed batch")
            want2, cnt2 = tab.page(k, cursors_of(want))
            assert (want2[tab.bad] == MISS).all() and (cnt2[tab.bad] == 0).all() and (cnt2[1::12] == cnt[1::12] - k).all()
            assert raw.call(CONTINUE) == 0
            page, got = raw.read()
            assert_pages(page, want2, "mixed batch, the next page, k = %d" % k)
            if counts:
                assert_counts(got, cnt2, "mixed batch, the next page")


# 5. sizes, and the smallest trees
@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_sizes_with_canaries(soup_ctx, n):
    tab = soup_table(0.8)
    want, cnt = tab.page(3)
    reps = -(-n // tab.n)
    raw = Raw(soup_ctx, np.tile(tab.b, (reps, 1))[:n], 3, pad=8)
    assert raw.call() == 0
    page, got = raw.read()
    assert_pages(page, np.tile(want, (reps, 1))[:n], "n = %d" % n)
    assert_counts(got, np.tile(cnt, reps)[:n], "n = %d" % n)


@pytest.mark.parametrize("count", (1, 2, 3))
def test_smallest_scenes(native_lib, count):
    """one triangle (the root is a leaf), two and three: empty slots fill the page"""
    few = soup_scene()[0][:count]
    rng = np.random.default_rng(count)
    c = few.reshape(-1, 3)[rng.integers(0, 3 * count, 128)] + (rng.random((128, 3)) - 0.5) * 0.04
    A = tris_around(rng, c, rng.random(128) * 0.2)
    A[::16] = few[0].mean(0) + np.float32([(-3, -3, 0), (5, -3, 0), (1, 6, 0)])  # eight large triangles through the first one's centroid
    tab = TriTable(queries_of_tris(A), few)
    cnt = tab.counts()
    assert (cnt > 0).sum() >= 5 and (cnt == 0).sum() >= 5
    r = context([few])
    try:
        assert r.bvh_info().triangle_count == count
        check(r, tab, 4, "%d triangles" % count)
    finally:
        r.close()


# 6. builders, masks, refit
@pytest.mark.parametrize("build", (B.BVH_BUILD_LBVH, B.BVH_BUILD_SAH, B.BVH_BUILD_PLOC, B.BVH_BUILD_SAH_DEVICE, B.BVH_BUILD_AUTO),
                         ids=("lbvh", "sah", "ploc", "sah_device", "auto"))
def test_every_builder_equals_the_brute_force(native_lib, build):
    r = context([soup_scene()[0]], build)
    try:
        check(r, soup_table(0.8), 4, "builder %d" % build, counts=True)
        check(r, soup_table(1.5), 16, "builder %d" % build, counts=False)
    finally:
        r.close()


def test_masks(native_lib):
    tris, tab = soup_scene()[0], soup_table(1.5)
    in_a = np.arange(len(tris)) < 1500
    none = np.zeros(len(tris), bool)
    assert not np.array_equal(tab.with_mask(in_a).page(4)[0], tab.with_mask(~in_a).page(4)[0])
    r = context([tris[:1500], tris[1500:]])
    try:
        check(r, tab, 4, "two meshes, no table", counts=True)
        r.set_instance_masks([0x01, 0x02])
        check(r, tab, 4, "plain call, both masks non-zero", counts=True)
        for mask, passes in ((0x01, in_a), (0x02, ~in_a), (0x03, None), (0xFC, none)):
            check(r, tab.with_mask(passes), 4, "mask 0x%02x" % mask, mask=mask)
            check(r, tab.with_mask(passes), 16, "mask 0x%02x" % mask, counts=False, mask=mask)
        _, got = r.overlap_triangles(tab.b, 0, counts=True, mask=0x02)
        assert_counts(got, tab.with_mask(~in_a).counts(), "k = 0 under a mask")
        r.set_instance_masks([0x00, 0xFF])
        check(r, tab.with_mask(~in_a), 4, "a mesh with mask 0 is invisible to the plain call")
        page = r.overlap_triangles(tab.b, 4)
        want_next = tab.with_mask(~in_a).page(4, cursors_of(page))[0]  # (before the call: a numpy page is resumed in place)
        assert_pages(r.overlap_triangles(tab.b, 4, resume=page), want_next, "the next page under a mask")
        r.set_instance_masks(None)
        check(r, tab, 4, "no table: every mesh passes every mask", counts=True, mask=0x01)
        with pytest.raises(capi.CapError):
            r.overlap_triangles(tab.b, 4, mask=0x100)
    finally:
        r.close()


def test_stale_until_refit_then_the_moved_vertices(native_lib):
    tris, tab = soup_scene()[0], soup_table(0.8)
    rng = np.random.default_rng(3)
    P = arrays(tris)[0]
    moved = (P + np.float32([0.05, -0.02, 0.03]) + (rng.random(P.shape) - 0.5).astype(np.float32) * np.float32(0.02)).astype(np.float32)
    tab_moved = TriTable(tab.b, moved.reshape(-1, 3, 3))
    assert not np.array_equal(tab_moved.page(4)[0], tab.page(4)[0])
    r = context([tris])
    try:
        check(r, tab, 4, "before the update", counts=True)
        r.update_vertices(positions=moved)
        with pytest.raises(capi.CapError, match="status 3.*cap_bvh_refit"):
            r.overlap_triangles(tab.b, 4, counts=True)
        r.refit_bvh()
        check(r, tab_moved, 4, "after the refit")
        r.build_bvh()
        check(r, tab_moved, 4, "after a rebuild", counts=True)
    finally:
        r.close()


# 7. errors and state, in cap_overlap_boxes' order
def test_argument_and_state_contract(native_lib):
    import torch
    tris, tab = soup_scene()[0], soup_table(0.8).first(128)
    L = capi.lib()
    n, k = 128, 4
    r = capi.Renderer(0)
    try:
        raw = Raw(r, tab.b, k, pad=8)
        P, O, Cn = raw.queries.data_ptr(), raw.page.data_ptr(), raw.cnt.data_ptr()
        opt = lambda *o: ctypes.byref(capi.TraceOptions(o[0], o[1], (ctypes.c_uint32 * 2)(*o[2:])))
        f = lambda p=P, m=n, kk=k, o=O, c=Cn, flags=0, options=None: L.cap_overlap_triangles(r.ctx, p, m, kk, o, c, flags, options)
        err = lambda rc, code, word: rc == code and word in L.cap_last_error()
        assert err(f(), ERR_STATE, b"cap_bvh_build")  # nothing uploaded
        r.upload_scene(*arrays(tris))
        assert f() == ERR_STATE and f(P, 0) == ERR_STATE  # uploaded, not built: the state comes before n == 0
        assert err(f(kk=17), ERR_INVALID_ARG, b"CAP_MULTI_MAX_K"), "the rules come before the state"
        r.build_bvh()
        assert err(L.cap_overlap_triangles(None, P, n, k, O, Cn, 0, None), ERR_INVALID_ARG, b"ctx is NULL")
        for flags in (0x04, 0x10, 0x20, 0x01, 0x80000000):
            assert err(f(options=opt(flags, 0, 0, 0)), ERR_INVALID_ARG, b"ray_flags")
        assert err(f(options=opt(0, 0, 1, 0)), ERR_INVALID_ARG, b"reserved") and err(f(options=opt(0, 0, 0, 7)), ERR_INVALID_ARG, b"reserved")
        assert err(f(options=opt(0, 0x100, 0, 0)), ERR_INVALID_ARG, b"exceeds 8 bits") and f(options=opt(0, 0xFFFFFFFF, 0, 0)) == ERR_INVALID_ARG
        assert err(f(flags=2), ERR_INVALID_ARG, b"unknown flags") and err(f(flags=0x80000000), ERR_INVALID_ARG, b"unknown flags")
        assert err(f(kk=17), ERR_INVALID_ARG, b"CAP_MULTI_MAX_K")
        assert err(f(kk=0), ERR_INVALID_ARG, b"k = 0 counts only") and err(f(kk=0, o=None, c=None), ERR_INVALID_ARG, b"k = 0 counts only")
        assert err(f(kk=0, o=None, flags=CONTINUE), ERR_INVALID_ARG, b"CAP_MULTI_CONTINUE needs k >= 1")
        assert err(f(None), ERR_INVALID_ARG, b"NULL") and err(f(o=None), ERR_INVALID_ARG, b"NULL")
        assert err(f(P + 4), ERR_INVALID_ARG, b"queries is not 16-byte aligned") and err(f(P + 8), ERR_INVALID_ARG, b"queries is not 16-byte aligned")
        assert err(f(o=O + 2), ERR_INVALID_ARG, b"triangles is not 4-byte aligned")
        assert err(f(c=Cn + 2), ERR_INVALID_ARG, b"counts is not 4-byte aligned")
        assert err(f(o=P), ERR_INVALID_ARG, b"overlap") and err(f(o=P + 48 * (n - 1) + 44), ERR_INVALID_ARG, b"overlap")  # page over queries
        assert err(f(O + 4 * k * (n - 1), n, k, O), ERR_INVALID_ARG, b"overlap")  # queries in the last page
        assert err(f(c=P + 48 * (n - 1) + 44), ERR_INVALID_ARG, b"overlap")  # counts over queries
        assert err(f(c=O + 4 * k * (n - 1) + 12), ERR_INVALID_ARG, b"overlap")  # counts over the page
        assert err(f(m=1 << 60, c=None), ERR_INVALID_ARG, b"address space")
        assert f(None, 0, k, None, None) == 0 and f(None, 0, 0, None, Cn) == 0  # nothing to do
        r.sync()
        torch.cuda.synchronize()
        assert raw.untouched(), "nothing is written on an error"
        assert raw.call() == 0
        page, got = raw.read()
        want, cnt = tab.page(k)
        assert_pages(page, want, "the call itself")
        assert_counts(got, cnt, "the call itself")
        only = Raw(r, tab.b, 0, pad=8)
        assert only.call() == 0  # k = 0: counts only
        assert_counts(only.read()[1], cnt, "k = 0")
        assert bool((only.page == CANARY).all())
        dev = torch.device("cuda", 0)
        for bad in (lambda: r.overlap_triangles(torch.zeros((4, 8), device=dev), 4),
                    lambda: r.overlap_triangles(raw.queries, 17),
                    lambda: r.overlap_triangles(raw.queries, -1),
                    lambda: r.overlap_triangles(raw.queries, 0),
                    lambda: r.overlap_triangles(raw.queries, 0, counts=True, resume=torch.zeros((n, 0), dtype=torch.int32, device=dev)),
                    lambda: r.overlap_triangles(raw.queries, 4, resume=torch.zeros((n, 4), device=dev)),
                    lambda: r.overlap_triangles(raw.queries, 4, resume=torch.zeros((n, 3), dtype=torch.int32, device=dev)),
                    lambda: r.overlap_triangles(tab.b, 4, resume=np.zeros((n, 3), np.int32))):
            with pytest.raises(capi.CapError):
                bad()
        # tensors in, tensors out, and the page resumed in place
        first = r.overlap_triangles(raw.queries, k)
        assert first.is_cuda and first.dtype == torch.int32 and first.shape == (n, k)
        assert_pages(first.cpu().numpy(), want, "tensors")
        second = r.overlap_triangles(raw.queries, k, resume=first)
        assert second.data_ptr() == first.data_ptr()
        assert_pages(second.cpu().numpy(), tab.page(k, cursors_of(want))[0], "tensors, the next page")
    finally:
        r.close()
