"""k-nearest / in-radius closest-point queries on the GPU (cap_closest_points_multi): every record of every page compared bit for bit, all
eight words, and every count, with the numpy float32 brute force of closest_multi_support.py over every triangle."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_multi_support import Table, all_miss, assert_counts, assert_pages, cursors_of, listed
from closest_point_support import MISS, arrays, around, bits, context, near_surface, needles, queries, soup, sphere
from multi_hit_support import stacked_quads

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 3
CONTINUE = capi.Renderer.MULTI_CONTINUE
CANARY = 0x7FC0BEEF  # a NaN pattern no record holds
B = capi.Renderer  # the CapBvhBuild values
INF = np.float32(np.inf)


def check(r, tab, k, what, counts=True, mask=None):
    """the first page of the table's queries, with and / or without counts, against the brute force"""
    want, cnt = tab.page(k)
    for c in ((False, True) if counts == "both" else (counts,)):
        if c:
            page, got = r.closest_points_multi(tab.q, k, counts=True, mask=mask)
            assert_counts(got, cnt, "%s, k = %d: counts" % (what, k))
        else:
            page = r.closest_points_multi(tab.q, k, mask=mask)
        assert page.shape == (tab.n, k, 8) and page.dtype == np.float32
        assert_pages(page, want, "%s, k = %d%s" % (what, k, ", counts" if c else ""))


class Raw:
    """the C call on torch buffers filled with canaries: `pad` points' worth of them behind the page and the counts"""

    def __init__(self, r, q, k, pad=4, counts=True):
        import torch
        self.r, self.n, self.k, self.L = r, len(q), k, capi.lib()
        dev = torch.device("cuda", 0)
        self.pts = torch.as_tensor(np.ascontiguousarray(q, np.float32), device=dev).contiguous()
        self.page = torch.full(((self.n + pad) * max(k, 1), 8), CANARY, dtype=torch.int32, device=dev)
        self.cnt = torch.full((self.n + pad,), CANARY, dtype=torch.int32, device=dev) if counts else None
        torch.cuda.synchronize()

    def call(self, flags=0, options=None):
        rc = self.L.cap_closest_points_multi(self.r.ctx, self.pts.data_ptr(), self.n, self.k, self.page.data_ptr() if self.k else None,
                                             self.cnt.data_ptr() if self.cnt is not None else None, flags, options)
        self.r.sync()
        return rc

    def read(self):
        """(page (n, k, 8) float32, counts (n,) or None); asserts the canaries behind both"""
        words = self.page.cpu().numpy().view(np.uint32)
        head = self.n * self.k
        assert (words[head:] == CANARY).all(), "nothing behind the last record"
        cnt = None
        if self.cnt is not None:
            c = self.cnt.cpu().numpy().view(np.uint32)
            assert (c[self.n:] == CANARY).all(), "nothing behind the last count"
            cnt = c[:self.n]
        return words[:head].view(np.float32).reshape(self.n, self.k, 8), cnt

    def untouched(self):
        return bool((self.page == CANARY).all()) and (self.cnt is None or bool((self.cnt == CANARY).all()))


@pytest.fixture(scope="module")
def soup_case():
    """5 000 small triangles (above the AUTO builder's threshold of 4 096) and 2 048 points inside and outside their box, half of them
    with a finite radius; the brute force's table, once"""
    rng = np.random.default_rng(7)
    tris = soup(rng, 5000, edge=0.05)
    q = queries(around(rng, tris, 2048, 0.5))
    q[1024:, 3] = rng.random(1024).astype(np.float32) * 0.2
    return tris, Table(q, tris)


@pytest.fixture(scope="module")
def soup_ctx(native_lib, soup_case):
    r = context([soup_case[0]])
    yield r
    r.close()


# 1. k = 1 is cap_closest_points
def test_k1_equals_closest_points(soup_case, soup_ctx):
    tris, tab = soup_case
    want, cnt = tab.page(1)
    hit = bits(want)[:, 0, 6] != MISS
    assert hit[:1024].all() and 100 < hit[1024:].sum() < 1000, "the radii split the second half into hits and misses"
    single = soup_ctx.closest_points(tab.q)
    assert_pages(single, want[:, 0], "cap_closest_points against the brute force")
    page = soup_ctx.closest_points_multi(tab.q, 1)
    assert page.shape == (2048, 1, 8)
    assert_pages(page[:, 0], single, "k = 1 against cap_closest_points")
    page, got = soup_ctx.closest_points_multi(tab.q, 1, counts=True)  # (the list kernel at K = 1)
    assert_pages(page[:, 0], single, "k = 1 with counts against cap_closest_points")
    assert_counts(got, cnt, "k = 1 counts")


# 2. both sides of every K bucket; empty, part-filled, just-filled and overfull pages
@pytest.fixture(scope="module")
def near_case():
    """the soup's triangles again (the same seed) with 512 points in and just around their box, radii up to 0.12: from no candidate to
    52 of them; the table, and the radii as fractions of that"""
    rng = np.random.default_rng(7)
    tris = soup(rng, 5000, edge=0.05)
    pts = around(rng, tris, 512, 0.05)
    unit = rng.random(512)
    return tris, Table(queries(pts, (unit * 0.12).astype(np.float32)), tris), unit


@pytest.mark.parametrize("k", (1, 2, 4, 5, 8, 9, 16))
def test_buckets_and_page_fill(soup_case, near_case, soup_ctx, k):
    tris, base, unit = near_case
    assert np.array_equal(tris, soup_case[0])
    tab = base.with_radius((unit * (0.12 if k <= 8 else 0.2)).astype(np.float32))
    c = tab.counts().astype(np.int64)
    classes = [(c == 0).sum(), ((c >= 1) & (c <= k)).sum(), ((c > k) & (c <= 3 * k)).sum(), (c > 3 * k).sum()]
    assert min(classes) >= 20, "k = %d: queries with 0, 1..k, k+1..3k and more candidates: %s" % (k, classes)
    check(soup_ctx, tab, k, "buckets", counts="both")


# 3. ties across page boundaries
def tie_case():
    _, tris = stacked_quads(40, 0.25)
    tris = np.concatenate([tris, tris])
    z = (np.arange(39) + 0.5) * 0.25
    pts = [(0.5, 0.5, zz) for zz in z[::4]] + [(0.25, 0.25, zz) for zz in z[1::4]] + [(0.75, 0.75, zz) for zz in z[2::4]]
    return tris, queries(pts, 0.8)


@pytest.fixture(scope="module")
def tie_ctx(native_lib):
    r = context([tie_case()[0]])
    yield r
    r.close()


@pytest.mark.parametrize("k", (1, 2, 3, 5, 16))
def test_ties_across_page_boundaries(tie_ctx, k):
    tris, q = tie_case()
    tab = Table(q, tris)
    full = [tab.candidates(i) for i in range(tab.n)]
    sizes = np.array([len(f) for f in full])
    assert sizes.min() >= 16 and sizes.max() <= 24 and max(len(np.unique(tab.d2[i, f])) for i, f in enumerate(full)) <= 3
    got_pages, seen = [], np.zeros(tab.n, np.int64)
    page = None
    for _ in range(40):
        page, cnt = tie_ctx.closest_points_multi(q, k, counts=True, resume=page)
        assert_counts(cnt, sizes - seen, "the remainder before page %d, k = %d" % (len(got_pages), k))
        got_pages.append(page.copy())
        seen += (bits(page)[..., 6] != MISS).sum(1)
        if all_miss(page):
            break
    assert all_miss(got_pages[-1]) and len(got_pages) == -(-24 // k) + 1
    for i, f in enumerate(full):
        rows = listed(got_pages, i)
        assert bits(rows)[:, 6].tolist() == f.tolist(), "k = %d point %d: every candidate once, in (dist2, id) order" % (k, i)
        assert_pages(rows, np.stack([tab.record(i, g) for g in f]), "k = %d point %d" % (k, i))
    # the same walk without counts (the k-th distance prunes) gives the same pages
    page = None
    for n, want in enumerate(got_pages):
        page = tie_ctx.closest_points_multi(q, k, resume=page)
        assert_pages(page, want, "k = %d page %d without counts" % (k, n))


# 4. builders
@pytest.mark.parametrize("build", (B.BVH_BUILD_LBVH, B.BVH_BUILD_SAH, B.BVH_BUILD_PLOC, B.BVH_BUILD_SAH_DEVICE, B.BVH_BUILD_AUTO),
                         ids=("lbvh", "sah", "ploc", "sah_device", "auto"))
def test_every_builder_equals_the_brute_force(native_lib, near_case, build):
    tris, tab, _ = near_case
    r = context([tris], build)
    try:
        check(r, tab, 4, "builder %d" % build)
    finally:
        r.close()


# 5. scenes built against the prune (those of test_closest_points_gpu.prune_scene)
def prune_scene(name):
    rng = np.random.default_rng(11)
    if name == "far from the origin":  # coordinates near 4 096, edges of 1e-2: the absolute rounding term dominates
        tris = soup(rng, 5000, edge=0.01, offset=4096.0)
        pts = np.concatenate([around(rng, tris, 384, 0.2), near_surface(rng, tris, 384, 2e-3)])
    elif name == "sphere from its centre":  # every subtree almost equally far: the bound is at its thinnest
        tris = sphere()
        assert 4500 < len(tris) < 5500
        pts = np.concatenate([np.zeros((1, 3)), rng.normal(size=(383, 3)) * 1e-3, rng.normal(size=(128, 3)) * 1e-6, rng.normal(size=(256, 3)) * 0.3]).astype(np.float32)
    elif name == "needles":  # aspect ratio 1e4
        tris = needles(rng, 5000, 0.2, 1e4)
        pts = np.concatenate([around(rng, tris, 384, 0.2), near_surface(rng, tris, 384, 1e-3)])
    else:
        raise KeyError(name)
    return tris, queries(pts)


@pytest.mark.parametrize("name", ("far from the origin", "sphere from its centre", "needles"))
def test_scenes_against_the_prune(native_lib, name):
    tris, q = prune_scene(name)
    tab = Table(q, tris)
    r = context([tris])
    try:
        for k in (4, 16):
            want, _ = tab.page(k)
            assert (bits(want)[..., 6] != MISS).all()
            check(r, tab, k, name, counts=False)  # the k-th bound does the pruning
            # the same with the radius a hair above the k-th distance: the bound starts thin instead of becoming so
            tight = tab.with_radius(np.sqrt(want[:, k - 1, 3]) * np.float32(1.000001))
            check(r, tight, k, name + ", tight radius", counts=False)
    finally:
        r.close()


# 6. radius edges
@pytest.mark.parametrize("k", (4, 16))
def test_radius_at_one_ulp_below_and_without(soup_case, soup_ctx, k):
    tab = soup_case[1].first(512).with_radius(INF)
    kth = tab.page(k)[0][:, k - 1, 3]
    at = np.sqrt(kth)
    assert at.dtype == np.float32 and np.isfinite(at).all()
    full = {}
    for name, radius in (("at", at), ("below", np.nextafter(at, np.float32(0))), ("inf", INF)):
        t = tab.with_radius(radius)
        full[name] = (t.counts() >= k).sum()
        check(soup_ctx, t, k, "radius " + name, counts="both")
    # sqrt rounds either way: fl(r * r) lands on both sides of the k-th dist2
    assert full["inf"] == 512 and 50 < full["at"] < 512 and full["below"] < full["at"]


def test_points_on_vertices_and_edges_with_radius_zero(native_lib, soup_case):
    _, quads = stacked_quads(8, 0.25)
    scene = np.concatenate([soup_case[0] + np.float32([2, 0, 0]), quads, quads])
    on_vertices = scene[::7].reshape(-1, 3)[:300]
    z = np.arange(8) * 0.25
    on_edges = np.concatenate([[(0.5, 0, k), (1, 0.5, k), (0.5, 0.5, k), (0, 0.25, k), (0.75, 1, k), (0, 0, k), (1, 1, k)] for k in z])
    q = queries(np.concatenate([on_vertices, on_edges]), 0.0)
    off = q.copy()
    off[:, 2] += np.float32(1e-3)  # ... and just off them: radius 0 admits nothing
    q = np.concatenate([q, off])
    tab = Table(q, scene)
    n = len(q) // 2
    c = tab.counts()
    assert (c[:n] >= 1).all() and (c[:n] >= 2).sum() >= 56 and (c[:n] == 4).sum() >= 24 and (c[n:] == 0).sum() > 0.9 * n
    want, _ = tab.page(4)
    ids = bits(want)[:n, :, 6].astype(np.int64)
    assert (want[:n, 0, 3] == 0).all() and (np.diff(ids[c[:n] == 4], axis=1) > 0).all(), "coincident candidates at dist2 == 0 come in id order"
    r = context([scene])
    try:
        for k in (1, 2, 4, 5):
            check(r, tab, k, "radius 0", counts="both")
    finally:
        r.close()


# 7. degenerate queries
@pytest.mark.parametrize("k", (1, 3, 16))
def test_degenerate_queries_between_good_ones(soup_case, soup_ctx, k):
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    q = soup_case[1].q[:96].copy()
    q[:, 3] = 0.3
    for j, (col, value) in enumerate(((0, nan), (1, inf), (2, -inf), (3, np.float32(-1.0)), (3, nan), (3, -inf), (0, -nan), (1, nan))):
        q[1 + 3 * j::24, col] = value
    tab = Table(q, soup_case[0])
    assert tab.bad.sum() == 32
    want, cnt = tab.page(k)
    miss = np.zeros(8, np.uint32)
    miss[6] = MISS
    assert (bits(want)[tab.bad] == miss).all() and (cnt[tab.bad] == 0).all() and (cnt[~tab.bad] > 0).sum() > 20
    for counts in (True, False):
        raw = Raw(soup_ctx, q, k, counts=counts)
        assert raw.call() == 0
        page, got = raw.read()
        assert_pages(page, want, "degenerate queries, k = %d" % k)
        if counts:
            assert_counts(got, cnt, "degenerate queries")
        want2, cnt2 = tab.page(k, cursors_of(want))
        assert (bits(want2)[tab.bad] == miss).all() and (cnt2[tab.bad] == 0).all() and (cnt2[~tab.bad] > 0).sum() > 5
        assert raw.call(CONTINUE) == 0
        page, got = raw.read()
        assert_pages(page, want2, "degenerate queries, the next page, k = %d" % k)
        if counts:
            assert_counts(got, cnt2, "degenerate queries, the next page")


# 8. sizes, and the smallest trees
@pytest.fixture(scope="module")
def size_case(near_case):
    tab = near_case[1]
    return (tab,) + tab.page(3)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_sizes_with_canaries(soup_ctx, size_case, n):
    tab, want, cnt = size_case
    reps = -(-n // tab.n)
    raw = Raw(soup_ctx, np.tile(tab.q, (reps, 1))[:n], 3, pad=8)
    assert raw.call() == 0
    page, got = raw.read()
    assert_pages(page, np.tile(want, (reps, 1, 1))[:n], "n = %d" % n)
    assert_counts(got, np.tile(cnt, reps)[:n], "n = %d" % n)


@pytest.mark.parametrize("count", (1, 2, 3))
def test_smallest_scenes(native_lib, soup_case, count):
    """one triangle (the root is a leaf), two (one node, one traversal leaf) and three: miss slots fill the page"""
    few = soup_case[0][:count]
    q = soup_case[1].q[:256].copy()
    q[:128, 3], q[128:, 3] = INF, 0.6
    tab = Table(q, few)
    want, cnt = tab.page(4)
    assert (cnt[:128] == count).all() and 0 < (cnt[128:] > 0).sum() < 128 and (bits(want)[:, 3, 6] == MISS).all()
    r = context([few])
    try:
        assert r.bvh_info().triangle_count == count
        check(r, tab, 4, "%d triangles" % count, counts="both")
        page, got = r.closest_points_multi(q, 0, counts=True)
        assert page.shape == (256, 0, 8)
        assert_counts(got, cnt, "k = 0")
    finally:
        r.close()


# 9. masks
def test_masks(native_lib, near_case):
    tris, tab, _ = near_case
    in_a = np.arange(len(tris)) < 2500
    none = np.zeros(len(tris), bool)
    assert not np.array_equal(bits(tab.with_mask(in_a).page(4)[0]), bits(tab.with_mask(~in_a).page(4)[0]))
    r = context([tris[:2500], tris[2500:]])
    try:
        check(r, tab, 4, "two meshes, no table")
        r.set_instance_masks([0x01, 0x02])
        check(r, tab, 4, "plain call, both masks non-zero")
        for mask, passes in ((0x01, in_a), (0x02, ~in_a), (0x03, None), (0xFC, none)):
            check(r, tab.with_mask(passes), 4, "mask 0x%02x" % mask, counts="both", mask=mask)
            check(r, tab.with_mask(passes), 16, "mask 0x%02x" % mask, counts=False, mask=mask)
        page, got = r.closest_points_multi(tab.q, 0, counts=True, mask=0x02)
        assert_counts(got, tab.with_mask(~in_a).counts(), "k = 0 under a mask")
        r.set_instance_masks([0x00, 0xFF])
        check(r, tab.with_mask(~in_a), 4, "a mesh with mask 0 is invisible to the plain call", counts="both")
        r.set_instance_masks(None)
        check(r, tab, 4, "no table: every mesh passes every mask", mask=0x01)
        with pytest.raises(capi.CapError):
            r.closest_points_multi(tab.q, 4, mask=0x100)
    finally:
        r.close()


# 10. refit
def test_stale_until_refit_then_the_moved_vertices(native_lib, near_case):
    tris, tab, _ = near_case
    rng = np.random.default_rng(3)
    P = arrays(tris)[0]
    moved = (P + np.float32([0.05, -0.02, 0.03]) + (rng.random(P.shape) - 0.5).astype(np.float32) * np.float32(0.02)).astype(np.float32)
    tab_moved = Table(tab.q, moved.reshape(-1, 3, 3))
    assert not np.array_equal(bits(tab_moved.page(4)[0]), bits(tab.page(4)[0]))
    r = context([tris])
    try:
        check(r, tab, 4, "before the update")
        r.update_vertices(positions=moved)
        with pytest.raises(capi.CapError, match="status 3.*cap_bvh_refit"):
            r.closest_points_multi(tab.q, 4, counts=True)
        r.refit_bvh()
        check(r, tab_moved, 4, "after the refit")
        r.build_bvh()
        check(r, tab_moved, 4, "after a rebuild")
    finally:
        r.close()


# 11. errors and state
def test_argument_and_state_contract(native_lib, near_case):
    import torch
    tris, tab = near_case[0], near_case[1].first(128)
    L = capi.lib()
    n, k = 128, 4
    r = capi.Renderer(0)
    try:
        raw = Raw(r, tab.q, k, pad=8)
        P, O, Cn = raw.pts.data_ptr(), raw.page.data_ptr(), raw.cnt.data_ptr()
        opt = lambda *o: ctypes.byref(capi.TraceOptions(o[0], o[1], (ctypes.c_uint32 * 2)(*o[2:])))
        f = lambda p=P, m=n, kk=k, o=O, c=Cn, flags=0, options=None: L.cap_closest_points_multi(r.ctx, p, m, kk, o, c, flags, options)
        err = lambda rc, code, word: rc == code and word in L.cap_last_error()
        assert err(f(), ERR_STATE, b"cap_bvh_build")  # nothing uploaded
        r.upload_scene(*arrays(tris))
        assert f() == ERR_STATE and f(P, 0) == ERR_STATE  # uploaded, not built: the state comes before n == 0
        assert err(f(kk=17), ERR_INVALID_ARG, b"CAP_MULTI_MAX_K"), "the rules come before the state"
        r.build_bvh()
        assert err(L.cap_closest_points_multi(None, P, n, k, O, Cn, 0, None), ERR_INVALID_ARG, b"ctx is NULL")
        for flags in (0x04, 0x10, 0x20, 0x01, 0x80000000):
            assert err(f(options=opt(flags, 0, 0, 0)), ERR_INVALID_ARG, b"ray_flags")
        assert err(f(options=opt(0, 0, 1, 0)), ERR_INVALID_ARG, b"reserved") and err(f(options=opt(0, 0, 0, 7)), ERR_INVALID_ARG, b"reserved")
        assert err(f(options=opt(0, 0x100, 0, 0)), ERR_INVALID_ARG, b"exceeds 8 bits") and f(options=opt(0, 0xFFFFFFFF, 0, 0)) == ERR_INVALID_ARG
        assert err(f(flags=2), ERR_INVALID_ARG, b"unknown flags") and err(f(flags=0x80000000), ERR_INVALID_ARG, b"unknown flags")
        assert err(f(kk=17), ERR_INVALID_ARG, b"CAP_MULTI_MAX_K")
        assert err(f(kk=0), ERR_INVALID_ARG, b"k = 0 counts only") and err(f(kk=0, o=None, c=None), ERR_INVALID_ARG, b"k = 0 counts only")
        assert err(f(kk=0, o=None, flags=CONTINUE), ERR_INVALID_ARG, b"CAP_MULTI_CONTINUE needs k >= 1")
        assert err(f(None), ERR_INVALID_ARG, b"NULL") and err(f(o=None), ERR_INVALID_ARG, b"NULL")
        assert err(f(P + 4), ERR_INVALID_ARG, b"points is not 16-byte aligned")
        assert err(f(o=O + 8), ERR_INVALID_ARG, b"output is not 16-byte aligned")
        assert err(f(c=Cn + 2), ERR_INVALID_ARG, b"counts is not 4-byte aligned")
        assert err(f(o=P), ERR_INVALID_ARG, b"overlap") and err(f(o=P + 16 * (n - 1)), ERR_INVALID_ARG, b"overlap")  # output over points
        assert err(f(O + 32 * k * (n - 1), n, k, O), ERR_INVALID_ARG, b"overlap")  # points in the last page
        assert err(f(c=P + 16 * (n - 1) + 12), ERR_INVALID_ARG, b"overlap")  # counts over points
        assert err(f(c=O + 32 * k * (n - 1) + 28), ERR_INVALID_ARG, b"overlap")  # counts over output
        assert err(f(m=1 << 58, kk=16, c=None), ERR_INVALID_ARG, b"address space")  # 2^58 points fit (2^62 B), 2^58 x 16 records do not
        assert f(None, 0, k, None, None) == 0 and f(None, 0, 0, None, Cn) == 0  # nothing to do
        r.sync()
        torch.cuda.synchronize()
        assert raw.untouched(), "nothing is written on an error"
        assert raw.call() == 0
        page, got = raw.read()
        want, cnt = tab.page(k)
        assert_pages(page, want, "the call itself")
        assert_counts(got, cnt, "the call itself")
        only = Raw(r, tab.q, 0, pad=8)
        assert only.call() == 0  # k = 0: counts only
        assert_counts(only.read()[1], cnt, "k = 0")
        assert bool((only.page == CANARY).all())
        dev = torch.device("cuda", 0)
        for bad in (lambda: r.closest_points_multi(torch.zeros((4, 3), device=dev), 4),
                    lambda: r.closest_points_multi(raw.pts, 17),
                    lambda: r.closest_points_multi(raw.pts, -1),
                    lambda: r.closest_points_multi(raw.pts, 0),
                    lambda: r.closest_points_multi(raw.pts, 0, counts=True, resume=torch.zeros((n, 0, 8), device=dev)),
                    lambda: r.closest_points_multi(raw.pts, 4, resume=torch.zeros((n, 4, 4), device=dev)),
                    lambda: r.closest_points_multi(raw.pts, 4, resume=torch.zeros((n, 3, 8), device=dev)),
                    lambda: r.closest_points_multi(tab.q, 4, resume=np.zeros((n, 3, 8), np.float32))):
            with pytest.raises(capi.CapError):
                bad()
    finally:
        r.close()


# 12. a render
def test_a_render_is_unchanged_by_a_query_between_its_batches(native_lib, bluenoise, cornell_path):
    geo = capi.Geometry(cornell_path)
    cam = capi.cornell_camera(64, 64)
    rng = np.random.default_rng(5)
    q = queries(rng.random((300, 3)).astype(np.float32) * 3.0 - np.float32([1.5, 0.5, 1.5]), 0.7)
    result = []
    for interleave in (False, True):
        r = capi.Renderer(0)
        try:
            r.upload_geometry(geo)
            r.upload_bluenoise(bluenoise)
            r.build_bvh()
            r.set_resolution(64, 64)
            r.set_camera(cam)
            r.render(0, 2, 2, capi.RENDER_AOV)
            if interleave:
                before = (bits(r.readback(capi.BUF_ACCUM_SUM)).copy(), r.stats().as_dict())
                page, cnt = r.closest_points_multi(q, 4, counts=True)
                again = r.closest_points_multi(q, 4, resume=page.copy())
                after = (bits(r.readback(capi.BUF_ACCUM_SUM)), r.stats().as_dict())
                assert np.array_equal(before[0], after[0])
                assert {k: v for k, v in before[1].items() if not k.startswith("ms_")} == {k: v for k, v in after[1].items() if not k.startswith("ms_")}
                P = geo.positions.reshape(-1, 3)
                tris = np.concatenate([P[geo.indices[int(d[3]):int(d[3]) + int(d[2])].astype(np.int64) + int(d[1])].reshape(-1, 3, 3) for d in geo.meshes])
                tab = Table(q, tris)
                want, want_cnt = tab.page(4)
                assert (want_cnt > 4).sum() > 50
                assert_pages(page, want, "the Cornell box (a scene of the exhaustive render path)")
                assert_counts(cnt, want_cnt, "the Cornell box")
                assert_pages(again, tab.page(4, cursors_of(want))[0], "the Cornell box, the next page")
            r.render(2, 2, 2, capi.RENDER_AOV)
            s = r.stats()
            result.append((bits(r.readback(capi.BUF_ACCUM_SUM)), (s.rays_primary, s.rays_extension, s.rays_shadow, s.shaded_vertices, s.frames)))
        finally:
            r.close()
    assert np.array_equal(result[0][0], result[1][0]) and result[0][1] == result[1][1]
