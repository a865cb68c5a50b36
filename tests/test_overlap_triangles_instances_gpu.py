"""Triangle overlap queries over instances on the GPU (cap_overlap_triangles_instances): every triangle, every instance and every count
compared bit for bit with the numpy float32 brute force of overlap_triangles_instances_support.py over every (query, instance,
triangle).  tests/test_overlap_triangles_instances.py asserts without a GPU that the cases below reach what they are named after."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_instances_support import live_of
from closest_point_support import arrays, bits, context, soup
from instance_support import extreme_transforms, flatten, grid_scene, regular_transforms, rotation, translations
from object_support import concat, scene_triangles, single_triangle, triangle_ranges
from overlap_support import assert_pages
from overlap_triangles_instances_support import (MISS, NONE, TriPairTable, affine, all_miss, assert_counts, assert_pair_pages, contact_instances,
                                                 counterexample, cursors_of, far_case, identity, ids_of, needle_case, odd_queries, pair_valid,
                                                 queries_near, queries_of_tris, soup_case, with_skip_pair)
from overlap_triangles_support import TriTable
from test_overlap_triangles_instances import grid_queries

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 3
CONTINUE = capi.Renderer.MULTI_CONTINUE
CANARY = 0x7FC0BEEF
B = capi.Renderer  # the CapBvhBuild values


def run(r, queries, k, counts=False, resume=None, mask=None):
    return r.overlap_triangles_instances(np.ascontiguousarray(queries, np.float32), k, counts=counts, resume=resume, mask=mask)


def check(r, tab, k, what, mask=None, counts=(False, True)):
    """the first pages of the table's queries, without and with counts, against the brute force; returns the expected pages"""
    want = tab.page(k)
    for c in counts:
        got = run(r, tab.b, k, counts=c, mask=mask)
        label = "%s, k = %d%s" % (what, k, ", with counts" if c else "")
        assert got[0].shape == (tab.n, k) and got[0].dtype == np.int32 and got[1].shape == (tab.n, k) and got[1].dtype == np.int32
        assert_pair_pages(got[:2], want[:2], label)
        if c:
            assert_counts(got[2], want[2], label)
    return want


def instanced(tris, M, build=None, **kw):
    r = context([tris], build)
    info = r.set_instances(M, **kw)
    return r, info


@pytest.fixture(scope="module")
def soup_ctx(native_lib):
    tris, M, _ = soup_case()
    r, info = instanced(tris, M)
    assert info.inert == 0
    yield r
    r.close()


# 1. both sides of every K bucket; empty, part-filled, just-filled and overfull pages
@pytest.mark.parametrize("k", (1, 2, 4, 5, 8, 9, 16))
def test_buckets_and_page_fill(soup_ctx, k):
    check(soup_ctx, soup_case()[2], k, "soup under 32 transforms")


def test_counts_only(soup_ctx):
    tab = soup_case()[2]
    tri, inst, cnt = run(soup_ctx, tab.b, 0, counts=True)
    assert tri.shape == (tab.n, 0) and inst.shape == (tab.n, 0)
    assert_counts(cnt, tab.counts(), "k = 0")
    with pytest.raises(capi.CapError):
        run(soup_ctx, tab.b, 0)
    with pytest.raises(capi.CapError):
        run(soup_ctx, tab.b, 0, counts=True, resume=(tri, inst))


# 2. paging to exhaustion: page boundaries inside an instance and between coincident instances
@pytest.mark.parametrize("k", (1, 3, 16))
def test_pages_to_exhaustion(native_lib, k):
    tris = soup(np.random.default_rng(5), 80, edge=0.4)
    M = np.stack([identity()[0], identity()[0], affine(np.eye(3), (8, 0, 0)), identity()[0]])
    tab = TriPairTable(queries_near(np.random.default_rng(6), M[:1], tris, 32, size=1.5, away=1000), M, tris)
    full = [tab.candidates(b) for b in range(tab.n)]
    sizes = np.array([len(f) for f in full])
    assert 18 <= sizes.max() <= 120 and (sizes == 0).any()
    r, _ = instanced(tris, M)
    try:
        for counts in (True, False):
            got_pages, seen, resume = [], np.zeros(tab.n, np.int64), None
            for _ in range(sizes.max() // k + 2):
                got = run(r, tab.b, k, counts=counts, resume=resume)
                if counts:
                    assert_counts(got[2], sizes - seen, "the remainder before page %d, k = %d" % (len(got_pages), k))
                got_pages.append((ids_of(got[0]).copy(), ids_of(got[1]).copy()))
                assert ((got_pages[-1][0] == MISS) == (got_pages[-1][1] == MISS)).all()
                seen += (got_pages[-1][0] != MISS).sum(1)
                resume = (got[0], got[1])
                if all_miss(got[0]):
                    break
            assert all_miss(got_pages[-1][0]) and len(got_pages) == -(-int(sizes.max()) // k) + 1, "the page after a short or a just-full page is empty"
            for b, f in enumerate(full):
                tri = np.concatenate([p[0][b] for p in got_pages])
                inst = np.concatenate([p[1][b] for p in got_pages])
                assert (inst[inst != MISS].astype(np.int64) * tab.t + tri[tri != MISS]).tolist() == f.tolist(), "k = %d query %d: every pair once, in order" % (k, b)
    finally:
        r.close()


# 3. crafted scenes
def test_contacts_under_a_translation_and_a_stretch(native_lib):
    tris, M, names, q, want = contact_instances()
    tab = TriPairTable(q, M, tris)
    r, _ = instanced(tris, M)
    try:
        tri, inst, cnt = run(r, q, 16, counts=True)
        for b, (name, pairs) in enumerate(zip(names, want)):
            t, i = ids_of(tri)[b], ids_of(inst)[b]
            assert list(zip(i[i != MISS].tolist(), t[t != MISS].tolist())) == pairs[:16] and cnt[b] == len(pairs), name
        for k in (1, 4, 16):
            check(r, tab, k, "stacked quads")
    finally:
        r.close()


@pytest.mark.parametrize("build", (B.BVH_BUILD_LBVH, B.BVH_BUILD_SAH, B.BVH_BUILD_SAH_DEVICE), ids=("lbvh", "sah", "sah_device"))
def test_the_counterexample_pair_is_listed(native_lib, build):
    """the scene that defeats the object-space prune of cap_overlap_instances (tests/test_overlap_triangles_instances.py asserts that it
    does): the coplanar segment under the 45-degree instance must be listed"""
    tris, M, q = counterexample()
    tab = TriPairTable(q, M, tris)
    assert tab.pairs(0) == [(0, 0)]
    r, _ = instanced(tris, M, build)
    try:
        tri, inst, cnt = run(r, q, 4, counts=True)
        assert ids_of(tri)[0].tolist() == [0, MISS, MISS, MISS] and ids_of(inst)[0].tolist() == [0, MISS, MISS, MISS] and cnt[0] == 1
        check(r, tab, 1, "the counterexample")
    finally:
        r.close()


@pytest.mark.parametrize("build", (B.BVH_BUILD_LBVH, B.BVH_BUILD_SAH, B.BVH_BUILD_SAH_DEVICE), ids=("lbvh", "sah", "sah_device"))
def test_every_builder_equals_the_brute_force(native_lib, build):
    tris, M, tab = soup_case()
    r, _ = instanced(tris, M, build)
    try:
        check(r, tab, 4, "builder %d" % build)
    finally:
        r.close()


@pytest.mark.parametrize("case", (far_case, needle_case), ids=("near 4096", "needles"))
def test_translations_near_4096_and_needles(native_lib, case):
    tris, M, tab = case()
    r, info = instanced(tris, M)
    try:
        assert info.inert == 0
        for k in (4, 16):
            check(r, tab, k, case.__name__)
    finally:
        r.close()


def test_extreme_transforms(native_lib):
    tris = soup(np.random.default_rng(42), 200, edge=0.2)
    M, must_be_inert = extreme_transforms()
    M = np.concatenate([M, regular_transforms(3)])
    live = live_of(M)
    assert not live[:len(must_be_inert)][must_be_inert].any() and live.sum() >= 4
    q = np.concatenate([queries_near(np.random.default_rng(43), M[live], tris, 120, size=1.0), odd_queries()[:2]])
    with np.errstate(all="ignore"):
        tab = TriPairTable(q, M, tris, pair_valid(len(M), len(tris), live))
    inst = tab.page(16)[1]
    assert live[inst[inst != MISS]].all() and len(np.unique(inst[inst != MISS])) == live.sum()
    r, info = instanced(tris, M)
    try:
        assert info.inert == (~live).sum()
        for k in (4, 16):
            check(r, tab, k, "extreme transforms")
    finally:
        r.close()


def test_sixteen_instances_at_one_place(native_lib):
    rng = np.random.default_rng(47)
    tris = soup(rng, 300, edge=0.1)
    M = np.stack([affine(rotation(rng) if j == 0 else np.eye(3), (0, 0, 0)) for j in range(16)])
    R = M[0, :, :3].astype(np.float64)
    for j in range(1, 16):
        a = 1e-3 * j
        M[j] = affine(R @ np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]), (0, 0, 0))
    tab = TriPairTable(queries_near(rng, M, tris, 128, size=0.5), M, tris)
    inst = tab.page(16)[1]
    rows = [len(np.unique(row[row != MISS])) for row in inst if (row != MISS).any()]
    assert np.median(rows) >= 3, "a query meets the same triangle in many instances"
    r, _ = instanced(tris, M)
    try:
        for k in (5, 16):
            check(r, tab, k, "16 instances at one place")
    finally:
        r.close()


# 4. far and non-finite queries in one batch, canaries behind all three outputs, and the next page
class Raw:
    """the C call on torch buffers filled with canaries: `pad` queries' worth of them behind both pages and the counts"""

    def __init__(self, r, queries, k, pad=4, counts=True):
        import torch
        self.r, self.n, self.k, self.L = r, len(queries), k, capi.lib()
        dev = torch.device("cuda", 0)
        self.q = torch.as_tensor(np.ascontiguousarray(queries, np.float32), device=dev).contiguous()
        self.tri = torch.full(((self.n + pad) * max(k, 1),), CANARY, dtype=torch.int32, device=dev)
        self.inst = torch.full(((self.n + pad) * max(k, 1),), CANARY, dtype=torch.int32, device=dev)
        self.cnt = torch.full((self.n + pad,), CANARY, dtype=torch.int32, device=dev) if counts else None
        torch.cuda.synchronize()

    def call(self, flags=0, options=None):
        rc = self.L.cap_overlap_triangles_instances(self.r.ctx, self.q.data_ptr(), self.n, self.k, self.tri.data_ptr() if self.k else None,
                                                    self.inst.data_ptr() if self.k else None, self.cnt.data_ptr() if self.cnt is not None else None, flags,
                                                    options)
        self.r.sync()
        return rc

    def read(self):
        """(triangles (n, k) uint32, instances (n, k) uint32, counts (n,) or None); asserts the canaries behind all of them"""
        t, i = self.tri.cpu().numpy().view(np.uint32), self.inst.cpu().numpy().view(np.uint32)
        head = self.n * self.k
        assert (t[head:] == CANARY).all() and (i[head:] == CANARY).all(), "nothing behind the last triangle or instance"
        cnt = None
        if self.cnt is not None:
            c = self.cnt.cpu().numpy().view(np.uint32)
            assert (c[self.n:] == CANARY).all(), "nothing behind the last count"
            cnt = c[:self.n]
        return t[:head].reshape(self.n, self.k), i[:head].reshape(self.n, self.k), cnt

    def untouched(self):
        return bool((self.tri == CANARY).all()) and bool((self.inst == CANARY).all()) and (self.cnt is None or bool((self.cnt == CANARY).all()))


def test_far_and_non_finite_queries_in_one_batch(soup_ctx):
    tris, M, tab = soup_case()
    q = np.concatenate([tab.b[:36], odd_queries()])
    q = q[np.random.default_rng(1).permutation(len(q))]
    with np.errstate(all="ignore"):
        t = TriPairTable(q, M, tris)
    cnt = t.counts()
    assert t.bad.sum() == 4 and (cnt > 48).sum() >= 1
    for k in (3, 16):
        want = t.page(k)
        assert (want[0][t.bad] == MISS).all() and (want[1][t.bad] == MISS).all()
        for counts in (True, False):
            raw = Raw(soup_ctx, q, k, counts=counts)
            assert raw.call() == 0
            tri, inst, got = raw.read()
            assert_pair_pages((tri, inst), want[:2], "mixed batch, k = %d" % k)
            if counts:
                assert_counts(got, cnt, "mixed batch")
            want2 = t.page(k, cursors_of(want[0], want[1]))
            assert (want2[2][t.bad] == 0).all() and (want2[2] == np.maximum(cnt.astype(np.int64) - k, 0)).all()
            assert raw.call(CONTINUE) == 0
            tri, inst, got = raw.read()
            assert_pair_pages((tri, inst), want2[:2], "mixed batch, the next page, k = %d" % k)
            if counts:
                assert_counts(got, want2[2], "mixed batch, the next page")


# 5. sizes, few instances, the smallest tree
@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_sizes_with_canaries(soup_ctx, n):
    tab = soup_case()[2]
    want = tab.page(3)
    reps = -(-n // tab.n)
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:n]
    raw = Raw(soup_ctx, tile(tab.b), 3, pad=8)
    assert raw.call() == 0
    tri, inst, got = raw.read()
    assert_pair_pages((tri, inst), (tile(want[0]), tile(want[1])), "n = %d" % n)
    assert_counts(got, tile(want[2]), "n = %d" % n)


@pytest.mark.parametrize("count", (1, 2, 3, 5))
def test_few_instances_and_a_one_triangle_scene(native_lib, count):
    """1, 2, 3 and 5 instances exercise the top level's padding; the one-triangle scene has a leaf for a root"""
    rng = np.random.default_rng(45)
    M = regular_transforms(6)[1:1 + count]
    for tris in (soup(rng, 100, edge=0.2), soup(rng, 1, edge=0.5)):
        tab = TriPairTable(np.concatenate([queries_near(rng, M, tris, 96, size=1.0), odd_queries()[:1]]), M, tris)
        c = tab.counts()
        assert (c == 0).sum() >= 5 and (c > 0).sum() >= 24
        r, _ = instanced(tris, M)
        try:
            assert r.bvh_info().triangle_count == len(tris)
            check(r, tab, 4, "%d instances, %d triangles" % (count, len(tris)))
        finally:
            r.close()


# 6. objects and masks
@pytest.mark.parametrize("count", (2, 3))
def test_objects(native_lib, count):
    rng = np.random.default_rng(43)
    parts = [arrays(soup(rng, 200, edge=0.2)), arrays(soup(rng, 150, edge=0.2, offset=0.5), soup(rng, 50, edge=0.3)), single_triangle()][:count]
    scene, ranges = concat(parts)
    tris = scene_triangles(scene)
    obj_of_tri = np.concatenate([np.full(n, k) for k, (f, n) in enumerate(triangle_ranges(scene[4], ranges))])
    M = regular_transforms(12)
    objects = np.arange(12) % count
    whole = TriPairTable(np.concatenate([queries_near(rng, M, tris, 160, size=1.0), odd_queries()[:1]]), M, tris)
    tab = whole.with_valid(pair_valid(12, len(tris), None, None, None, None, objects, obj_of_tri))
    tri, inst, _ = tab.page(8)
    hit = inst != MISS
    assert (obj_of_tri[tri[hit]] == objects[inst[hit]]).all() and len(np.unique(objects[inst[hit]])) == count, "every object answers somewhere"
    assert not np.array_equal(whole.page(8)[0], tri)
    r = capi.Renderer(0)
    try:
        r.upload_scene(*scene)
        r.build_bvh()
        r.set_instances(M)
        check(r, whole, 8, "no object table: every instance shows the scene")
        r.set_objects(ranges)
        with pytest.raises(capi.CapError, match="status 3.*cap_instances_set"):
            run(r, whole.b, 8)  # set_objects dropped the instance table
        r.set_instances(M, objects=objects)
        check(r, tab, 8, "%d objects" % count)
        check(r, tab, 3, "%d objects" % count)
    finally:
        r.close()


def test_instance_mesh_and_call_masks(native_lib):
    rng = np.random.default_rng(44)
    a, b = soup(rng, 150, edge=0.2), soup(rng, 150, edge=0.2)
    tris = np.concatenate([a, b])
    M = regular_transforms(8)
    imasks = np.uint32([0x01, 0x02, 0x04, 0xFF, 0x03, 0x00, 0x01, 0x02])
    mesh_of_tri = (np.arange(300) >= 150).astype(np.int64)
    base = TriPairTable(np.concatenate([queries_near(rng, M, tris, 192, size=1.2), odd_queries()[:1]]), M, tris)

    def ref(inst_masks=None, mesh_masks=None, mask=None):
        tm = None if mesh_masks is None else np.uint32(mesh_masks)[mesh_of_tri]
        return base.with_valid(pair_valid(8, 300, None, inst_masks, tm, mask))

    r = context([a, b])
    try:
        r.set_instances(M, masks=imasks)
        inst = ref(imasks).page(16)[1]
        assert (inst != 5).all() and not np.array_equal(inst, ref().page(16)[1])
        check(r, ref(imasks), 16, "instance masks")
        check(r, ref(imasks, None, 0x01), 4, "instance masks and the call's mask", mask=0x01)
        check(r, ref(imasks, None, 0x08), 4, "a call mask only 0xFF passes", mask=0x08)
        r.set_instance_masks([0x05, 0x02])
        check(r, ref(imasks, [0x05, 0x02]), 16, "instance and mesh masks")
        check(r, ref(imasks, [0x05, 0x02], 0x06), 5, "instance, mesh and call masks", mask=0x06)
        r.set_instance_masks([0x00, 0xFF])
        only_b = ref(imasks, [0x00, 0xFF])
        tri, inst, _ = only_b.page(4)
        assert (tri[inst != MISS] >= 150).all() and (inst != MISS).any()
        check(r, only_b, 4, "a mesh with mask 0 is invisible")
        first = run(r, base.b, 4)
        want_next = only_b.page(4, cursors_of(first[0], first[1]))  # (before the call: numpy pages are resumed in place)
        assert_pair_pages(run(r, base.b, 4, resume=first)[:2], want_next[:2], "the next page under the masks")
        r.set_instance_masks([0x00, 0x00])
        tri, inst, cnt = run(r, base.b, 4, counts=True)
        assert all_miss(tri) and all_miss(inst) and (cnt == 0).all()
        with pytest.raises(capi.CapError):
            run(r, base.b, 4, mask=0x100)
    finally:
        r.close()


# 7. the skip pair, through instance_triangle_queries
def test_the_skip_pair_of_placed_triangles(native_lib):
    rng = np.random.default_rng(50)
    tris = soup(rng, 300, edge=0.25)
    M = regular_transforms(6).copy()
    M[4] = M[1]  # a coincident copy: the placed triangle meets its twin, which the skip pair must leave in
    inst, ids = rng.integers(0, 6, 200), rng.integers(0, 300, 200)
    inst[:20], inst[20:40] = 1, 4
    r, _ = instanced(tris, M)
    try:
        q = r.instance_triangle_queries(M, inst, ids)
        tab = TriPairTable(q, M, tris)
        plain = TriPairTable(with_skip_pair(q, np.zeros(200), np.full(200, NONE)), M, tris)
        assert (plain.counts() == tab.counts() + 1).all(), "every placed triangle meets itself, and only that pair goes"
        assert all((4, int(ids[n])) in tab.pairs(n) for n in range(20)) and all((1, int(ids[n])) in tab.pairs(n) for n in range(20, 40))
        assert (tab.counts() > 1).sum() >= 40
        for k in (4, 16):
            check(r, tab, k, "placed triangles with their skip pair")
        check(r, plain, 4, "skip = 0xFFFFFFFF with pad0 = 0 skips nothing")
        # the other instance's copy of the same id, an id beyond the scene and an instance beyond the table skip nothing
        for i2, g2 in ((((inst + 1) % 6), ids), (inst, ids + 300), (inst + 6, ids)):
            other = TriPairTable(with_skip_pair(q, i2, g2), M, tris)
            assert (other.counts() >= tab.counts()).all()
            check(r, other, 4, "a skip pair that names something else", counts=(True,))
        # paging passes over the skipped pair
        first = run(r, q, 2)
        assert_pair_pages(run(r, q, 2, resume=first)[:2], tab.page(2, cursors_of(*tab.page(2)[:2]))[:2], "the next page")
    finally:
        r.close()


# 8. the identities on the device
def test_one_identity_instance_is_cap_overlap_triangles(native_lib):
    tris = soup(np.random.default_rng(48), 500, edge=0.2)
    q = np.concatenate([queries_near(np.random.default_rng(49), identity(), tris, 192, size=0.8), queries_of_tris(tris[:64])])
    q = with_skip_pair(q, np.zeros(256), np.concatenate([np.full(192, NONE), np.arange(64)]))  # skip_instance = 0
    flat = TriTable(q, tris)
    r, _ = instanced(tris, identity())
    try:
        for k in (4, 16):
            page, cnt = r.overlap_triangles(q, k, counts=True)
            tri, inst, got = run(r, q, k, counts=True)
            assert_pages(tri, page, "k = %d: the triangles of the flat query" % k)
            assert_pages(page, flat.page(k)[0], "k = %d: the flat query itself" % k)
            assert_counts(got, cnt, "k = %d" % k)
            assert ((ids_of(inst) == 0) == (ids_of(tri) != MISS)).all() and ((ids_of(inst) == MISS) == (ids_of(tri) == MISS)).all()
        assert (flat.counts()[192:] > 0).sum() > 20 and not (ids_of(page)[192:] == np.arange(64)[:, None]).any()
    finally:
        r.close()


def test_translations_on_a_grid_give_the_flattened_scene(native_lib):
    rng = np.random.default_rng(8)
    scene, tris = grid_scene()
    T = rng.integers(-32 * 16, 32 * 16 + 1, (6, 3)) / 16.0
    q = grid_queries(rng, T)
    r = capi.Renderer(0)
    f = capi.Renderer(0)
    try:
        r.upload_scene(*scene)
        r.build_bvh()
        r.set_instances(translations(T))
        f.upload_scene(*flatten(scene, T))
        f.build_bvh()
        page, cnt = f.overlap_triangles(q, 16, counts=True)
        tri, inst, got = run(r, q, 16, counts=True)
        hit = ids_of(tri) != MISS
        assert hit.sum() > 100 and len(np.unique(ids_of(inst)[hit])) == 6
        flat_ids = np.where(hit, ids_of(inst).astype(np.int64) * len(tris) + ids_of(tri), MISS).astype(np.uint32)
        assert_pages(flat_ids, page, "flat id = i T + g")
        assert_counts(got, cnt, "the flattened scene's counts")
    finally:
        r.close()
        f.close()


def test_scaling_by_a_power_of_two_changes_nothing(native_lib, soup_ctx):
    tris, M, tab = soup_case()
    want = check(soup_ctx, tab.first(128), 8, "unscaled")
    for j in (-20, 7):
        s = np.float32(2.0 ** j)
        r, _ = instanced(tris, (M * s).astype(np.float32))
        try:
            scaled = tab.b[:128].copy()
            scaled[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] *= s
            got = run(r, scaled, 8, counts=True)
            assert_pair_pages(got[:2], want[:2], "everything x 2^%d" % j)
            assert_counts(got[2], want[2], "everything x 2^%d" % j)
        finally:
            r.close()


# 9. state and arguments
def test_state_refit_rebuild_and_replaced_tables(native_lib):
    rng = np.random.default_rng(46)
    tris = soup(rng, 300, edge=0.2)
    M, M2 = regular_transforms(8), regular_transforms(8, seed=77)
    q = np.concatenate([queries_near(rng, M, tris, 96, size=1.0), queries_near(rng, M2, tris, 96, size=1.0)])
    P = arrays(tris)[0]
    moved = (P + np.float32([0.05, -0.02, 0.03]) + (rng.random(P.shape) - 0.5).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    tab, tab_moved, tab2 = TriPairTable(q, M, tris), TriPairTable(q, M, moved.reshape(-1, 3, 3)), TriPairTable(q, M2, tris)
    assert not np.array_equal(tab.page(4)[0], tab_moved.page(4)[0]) and not np.array_equal(tab.page(4)[1], tab2.page(4)[1])
    r = context([tris])
    try:
        with pytest.raises(capi.CapError, match="status 3.*cap_instances_set"):
            run(r, q, 4)
        r.set_instances(M)
        check(r, tab, 4, "the first table")
        r.set_instances(M2)
        check(r, tab2, 4, "a second set_instances replaces the answers")
        r.set_instances(M)
        r.update_vertices(positions=moved)
        with pytest.raises(capi.CapError, match="status 3.*cap_bvh_refit"):
            run(r, q, 4)
        r.refit_bvh()
        check(r, tab_moved, 4, "after the refit")
        r.build_bvh()
        check(r, tab_moved, 4, "after a rebuild")
        r.set_instances(None)
        with pytest.raises(capi.CapError, match="status 3"):
            run(r, q, 4)
    finally:
        r.close()


def test_argument_contract(native_lib):
    import torch
    tris, M, tab = soup_case()
    tab = tab.first(128)
    dev = torch.device("cuda", 0)
    L = capi.lib()
    n, k = 128, 4
    want = tab.page(k)
    r = capi.Renderer(0)
    try:
        raw = Raw(r, tab.b, k, pad=8)
        P, O, I, Cn = raw.q.data_ptr(), raw.tri.data_ptr(), raw.inst.data_ptr(), raw.cnt.data_ptr()
        opts = lambda *o: ctypes.byref(capi.TraceOptions(o[0], o[1], (ctypes.c_uint32 * 2)(*o[2:])))
        call = lambda p=P, m=n, kk=k, o=O, i=I, c=Cn, flags=0, options=None: L.cap_overlap_triangles_instances(r.ctx, p, m, kk, o, i, c, flags, options)
        bad = lambda *a, **kw: call(*a, **kw) == ERR_INVALID_ARG
        assert call() == ERR_STATE and b"cap_bvh_build" in L.cap_last_error()  # nothing uploaded
        r.upload_scene(*arrays(tris))
        assert bad(kk=17) and b"CAP_MULTI_MAX_K" in L.cap_last_error(), "the rules come before the state"
        r.build_bvh()
        assert call() == ERR_STATE and b"cap_instances_set" in L.cap_last_error() and call(P, 0) == ERR_STATE  # the state comes before n == 0
        r.set_instances(M)
        assert L.cap_overlap_triangles_instances(None, P, n, k, O, I, Cn, 0, None) == ERR_INVALID_ARG
        for flags in (0x04, 0x10, 0x20, 0x01, 0x80000000):
            assert bad(options=opts(flags, 0, 0, 0)) and b"ray_flags" in L.cap_last_error()
        assert bad(options=opts(0, 0, 1, 0)) and bad(options=opts(0, 0, 0, 7)) and b"reserved" in L.cap_last_error()
        assert bad(options=opts(0, 0x100, 0, 0)) and b"exceeds 8 bits" in L.cap_last_error() and bad(options=opts(0, 0xFFFFFFFF, 0, 0))
        assert bad(flags=2) and bad(flags=0x80000000) and b"unknown flags" in L.cap_last_error()
        assert bad(kk=17) and b"CAP_MULTI_MAX_K" in L.cap_last_error()
        assert bad(kk=0) and bad(kk=0, i=None) and bad(kk=0, o=None) and bad(kk=0, o=None, i=None, c=None) and b"k = 0 counts only" in L.cap_last_error()
        assert bad(kk=0, o=None, i=None, flags=CONTINUE) and b"CAP_MULTI_CONTINUE" in L.cap_last_error()
        assert bad(None) and bad(o=None) and bad(i=None) and b"NULL" in L.cap_last_error()
        assert bad(P + 4) and b"queries is not 16-byte aligned" in L.cap_last_error() and bad(P + 8)
        assert bad(o=O + 2) and b"triangles is not 4-byte aligned" in L.cap_last_error()
        assert bad(i=I + 2) and b"instances is not 4-byte aligned" in L.cap_last_error()
        assert bad(c=Cn + 2) and b"counts is not 4-byte aligned" in L.cap_last_error()
        assert bad(o=P) and bad(o=P + 48 * (n - 1) + 44) and bad(i=P) and b"overlap" in L.cap_last_error()  # pages over the queries
        assert bad(O + 4 * k * (n - 1), n, k, O) and bad(i=O + 4 * k * n - 4) and bad(o=I + 4 * k * n - 4) and b"overlap" in L.cap_last_error()
        assert bad(c=P + 48 * (n - 1) + 44) and bad(c=O + 4 * k * n - 4) and bad(c=I) and bad(i=Cn + 4 * n - 4) and b"overlap" in L.cap_last_error()
        assert bad(m=1 << 60, c=None) and b"address space" in L.cap_last_error()
        assert call(None, 0, k, None, None, None) == 0 and call(None, 0, 0, None, None, Cn) == 0  # nothing to do
        r.sync()
        torch.cuda.synchronize()
        assert raw.untouched(), "nothing is written on an error"
        assert raw.call(options=opts(0, 0, 0, 0)) == 0  # the all-zero options are the plain call
        tri, inst, got = raw.read()
        assert_pair_pages((tri, inst), want[:2], "the call itself")
        assert_counts(got, want[2], "the call itself")
        only = Raw(r, tab.b, 0, pad=8)
        assert only.call() == 0  # k = 0: counts only
        assert_counts(only.read()[2], want[2], "k = 0")
        assert bool((only.tri == CANARY).all()) and bool((only.inst == CANARY).all())
        assert call(c=None) == 0
        r.sync()
        for wrong in (lambda: r.overlap_triangles_instances(torch.zeros((4, 8), device=dev), 4),
                      lambda: r.overlap_triangles_instances(raw.q, 17),
                      lambda: r.overlap_triangles_instances(raw.q, -1),
                      lambda: r.overlap_triangles_instances(raw.q, 0),
                      lambda: r.overlap_triangles_instances(raw.q, 4, resume=torch.zeros((n, 4), dtype=torch.int32, device=dev)),
                      lambda: r.overlap_triangles_instances(raw.q, 4, resume=(torch.zeros((n, 4), dtype=torch.int32, device=dev), torch.zeros((n, 3), dtype=torch.int32, device=dev))),
                      lambda: r.overlap_triangles_instances(raw.q, 4, resume=(torch.zeros((n, 4), device=dev), torch.zeros((n, 4), dtype=torch.int32, device=dev)))):
            with pytest.raises(capi.CapError):
                wrong()
        # tensors in, tensors out, and the pages resumed in place
        first = r.overlap_triangles_instances(raw.q, k)
        assert first[0].is_cuda and first[0].dtype == torch.int32 and first[0].shape == (n, k) and first[1].shape == (n, k)
        assert_pair_pages((first[0].cpu().numpy(), first[1].cpu().numpy()), want[:2], "tensors")
        second = r.overlap_triangles_instances(raw.q, k, resume=first)
        assert second[0].data_ptr() == first[0].data_ptr() and second[1].data_ptr() == first[1].data_ptr()
        assert_pair_pages((second[0].cpu().numpy(), second[1].cpu().numpy()), tab.page(k, cursors_of(want[0], want[1]))[:2], "tensors, the next page")
    finally:
        r.close()


# 10. render isolation
def test_a_render_is_unchanged_by_a_query_between_its_batches(native_lib, bluenoise, cornell_path):
    geo = capi.Geometry(cornell_path)
    cam = capi.cornell_camera(64, 64)
    rng = np.random.default_rng(5)
    M = np.stack([identity()[0], affine(rotation(rng) * 0.5, (300, 100, -200)), affine(np.diag([1.0, 2.0, 0.5]), (-50, 20, 10))])
    P = geo.positions.reshape(-1, 3)
    tris = np.concatenate([P[geo.indices[int(d[3]):int(d[3]) + int(d[2])].astype(np.int64) + int(d[1])].reshape(-1, 3, 3) for d in geo.meshes])
    q = queries_near(rng, M, tris, 200, size=0.5)
    result = []
    for interleave in (False, True):
        r = capi.Renderer(0)
        try:
            r.upload_geometry(geo)
            r.upload_bluenoise(bluenoise)
            r.build_bvh()
            r.set_instances(M)
            r.set_resolution(64, 64)
            r.set_camera(cam)
            r.render(0, 2, 2, capi.RENDER_AOV)
            if interleave:
                before = (bits(r.readback(capi.BUF_ACCUM_SUM)).copy(), r.stats().as_dict())
                got = r.overlap_triangles_instances(q, 8, counts=True)
                after = (bits(r.readback(capi.BUF_ACCUM_SUM)), r.stats().as_dict())
                assert np.array_equal(before[0], after[0])
                assert {k: v for k, v in before[1].items() if not k.startswith("ms_")} == {k: v for k, v in after[1].items() if not k.startswith("ms_")}
                want = TriPairTable(q, M, tris).page(8)
                assert (want[2] > 0).sum() > 60 and len(np.unique(want[1])) == 4
                assert_pair_pages(got[:2], want[:2], "the Cornell box under three instances")
                assert_counts(got[2], want[2], "the Cornell box under three instances")
            r.render(2, 2, 2, capi.RENDER_AOV)
            s = r.stats()
            result.append((bits(r.readback(capi.BUF_ACCUM_SUM)), (s.rays_primary, s.rays_extension, s.rays_shadow, s.shaded_vertices, s.frames)))
        finally:
            r.close()
    assert np.array_equal(result[0][0], result[1][0]) and result[0][1] == result[1][1]
