"""k-nearest / in-radius closest-point queries over instances on the GPU (cap_closest_instances_multi): every record word, every instance
and every count compared bit for bit with the numpy float32 brute force of closest_instances_multi_support.py over every (instance,
triangle) pair."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_instances_multi_support import PairTable, all_miss, assert_counts, assert_pair_pages, cursors_of, pages, tie_case
from closest_instances_support import (affine, identity, instance_box_points, live_of, pair_valid, world_hull_points, world_points_near)
from closest_point_support import MISS, arrays, bits, context, queries, soup
from instance_support import extreme_transforms, regular_transforms, rotation
from object_support import concat, scene_triangles, single_triangle, triangle_ranges
from test_closest_instances_gpu import prune_scene

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 3
CONTINUE = capi.Renderer.MULTI_CONTINUE
CANARY = 0x7FC0BEEF  # a NaN pattern no record holds
B = capi.Renderer  # the CapBvhBuild values


def run(r, q, k, counts=False, resume=None, mask=None):
    return r.closest_instances_multi(np.ascontiguousarray(q, np.float32), k, counts=counts, resume=resume, mask=mask)


def check(r, tab, k, what, mask=None, counts=(False, True)):
    """the call on tab's points against tab's expected pages, pruned by the k-th distance (no counts) and by the radius alone (counts).
    Returns the expected (records, instances, counts)."""
    want = tab.page(k)
    for c in counts:
        got = run(r, tab.q, k, counts=c, mask=mask)
        label = "%s, k = %d%s" % (what, k, ", with counts" if c else "")
        assert_pair_pages(got[:2], want[:2], label)
        if c:
            assert_counts(got[2], want[2], label)
    return want


def kth_radius(tab, k, scale=1.000001):
    """per point the radius a hair above the distance of its k-th pair (tab without a radius); +inf where it has fewer pairs"""
    radius = np.full(tab.n, np.inf, np.float32)
    for i in range(tab.n):
        ids = tab.candidates(i)
        if len(ids) >= k:
            radius[i] = np.sqrt(tab.d2[i, ids[k - 1]]) * np.float32(scale)
    return radius


# 1. the brute force: a 600-triangle soup under 32 transforms
REACH = (None, 1, 2, 3, 4, 6, 9, 14, 17, 30, 47, 49, 70, 200)  # how many pairs a point's radius reaches; None: half way to the nearest


@pytest.fixture(scope="module")
def brute_case():
    """256 points, half uniform in the instances' grown boxes and half near world surfaces, point i's radius a hair above the distance
    of its REACH[i mod 14]-th nearest pair; the dist2 table, once"""
    rng = np.random.default_rng(41)
    tris = soup(rng, 600, edge=0.1)
    M = regular_transforms(32)
    q = queries(np.concatenate([instance_box_points(rng, M, tris, 128, 0.1), world_points_near(rng, M, tris, 128, 0.02)]))
    free = PairTable(q, M, tris)
    radius = np.zeros(len(q), np.float32)
    for i in range(len(q)):
        d, m = np.sort(free.d2[i]), REACH[i % len(REACH)]
        radius[i] = np.sqrt(d[0]) * np.float32(0.5) if m is None else np.sqrt(d[m - 1]) * np.float32(1.000001)
    return tris, M, free.with_radius(radius)


@pytest.fixture(scope="module")
def brute_context(native_lib, brute_case):
    tris, M, _ = brute_case
    r = context([tris])
    info = r.set_instances(M)
    assert info.inert == 0
    yield r
    r.close()


def test_k1_is_cap_closest_instances(brute_case, brute_context):
    _, _, tab = brute_case
    r = brute_context
    single = r.closest_instances(tab.q)
    assert 0 < (single[1] >= 0).sum() < tab.n
    rec, inst = run(r, tab.q, 1)
    assert_pair_pages((rec[:, 0], inst[:, 0]), single, "k = 1 against cap_closest_instances")
    rec, inst, cnt = run(r, tab.q, 1, counts=True)  # (the list kernel at K = 1)
    assert_pair_pages((rec[:, 0], inst[:, 0]), single, "k = 1 with counts against cap_closest_instances")
    assert ((cnt > 0) == (single[1] >= 0)).all()


@pytest.mark.parametrize("k", (1, 2, 4, 5, 8, 9, 16))
def test_pages_and_counts_equal_the_brute_force(brute_case, brute_context, k):
    _, _, tab = brute_case
    c = tab.counts()
    assert (c == 0).sum() >= 8 and ((c >= 1) & (c <= k)).sum() >= 8 and ((c > k) & (c <= 3 * k)).sum() >= 8 and (c > 3 * k).sum() >= 8, \
        "points with no pair, with a short page, with up to three pages and with more"
    _, inst, _ = tab.page(k)
    assert len(np.unique(inst[inst >= 0])) >= 8, "pairs of many instances in the pages"
    check(brute_context, tab, k, "soup under 32 transforms")


# 2. paging to exhaustion over ties that span instances
@pytest.mark.parametrize("k", (1, 2, 3, 5, 16))
def test_paging_walks_every_pair_once(native_lib, k):
    tris, M, q = tie_case()
    tab = PairTable(q, M, tris)
    sizes = tab.counts()
    assert sizes.min() >= 16 and sizes.max() <= 24
    walk = pages(tab, k)
    assert all_miss(walk[-1][0]) and not all_miss(walk[-2][0]) and len(walk) >= 24 // k + 1
    r = context([tris])
    try:
        r.set_instances(M)
        for counts in (True, False):
            got = run(r, q, k, counts=counts)
            for n, (rec, inst, cnt) in enumerate(walk):
                what = "k = %d page %d%s" % (k, n, ", with counts" if counts else "")
                assert_pair_pages(got[:2], (rec, inst), what)
                if counts:
                    assert_counts(got[2], cnt, what)  # the remainder, on every page
                if n + 1 < len(walk):
                    got = run(r, q, k, counts=counts, resume=(got[0], got[1]))
            assert all_miss(got[0]) and (got[1] == -1).all()
    finally:
        r.close()


# 3. the three builders
@pytest.mark.parametrize("build", (B.BVH_BUILD_LBVH, B.BVH_BUILD_SAH, B.BVH_BUILD_SAH_DEVICE), ids=("lbvh", "sah", "sah_device"))
def test_every_builder_equals_the_brute_force(native_lib, brute_case, build):
    tris, M, tab = brute_case
    r = context([tris], build)
    try:
        r.set_instances(M)
        check(r, tab, 4, "builder %d" % build)
    finally:
        r.close()


# 4. scenes built against the prune
@pytest.mark.parametrize("name", ("translations near 4096", "sphere from the image of its centre", "points 1e5 away", "16 instances at one place"))
def test_scenes_against_the_prune(native_lib, name):
    tris, M, q = prune_scene(name)
    free = PairTable(q, M, tris)
    r = context([tris])
    try:
        info = r.set_instances(M)
        assert info.inert == 0
        for k in (4, 16):
            want = check(r, free, k, name, counts=(False,))
            assert not (bits(want[0])[..., 6] == MISS).any(), "full pages everywhere"
            tight = free.with_radius(kth_radius(free, k))  # the bound starts thin instead of becoming so
            assert (tight.counts() >= k).all() and np.isfinite(tight.r2).all()
            check(r, tight, k, name + ", tight radius")
    finally:
        r.close()


# 5. the radius at, one ulp below and one ulp above the k-th pair's distance, and no radius
def test_radius_at_beside_and_without_the_kth_distance(brute_case, brute_context):
    _, _, tab = brute_case
    free = tab.with_radius(np.inf)
    k = 4
    at, below, above = (np.zeros(tab.n, np.float32) for _ in range(3))
    exact = np.zeros(tab.n, bool)
    for i in range(tab.n):
        d2 = free.d2[i, free.candidates(i)[k - 1]]
        root = np.sqrt(d2)
        for cand in (root, np.nextafter(root, np.float32(0)), np.nextafter(root, np.float32(np.inf))):
            if cand * cand == d2:
                at[i], exact[i] = cand, True
        if not exact[i]:
            at[i] = root
        below[i], above[i] = np.nextafter(at[i], np.float32(0)), np.nextafter(at[i], np.float32(np.inf))
    assert exact.sum() > tab.n // 4, "radii whose square IS the k-th dist2"
    t_at, t_below, t_above = free.with_radius(at), free.with_radius(below), free.with_radius(above)
    c_at, c_below, c_above = t_at.counts(), t_below.counts(), t_above.counts()
    assert (c_at[exact] >= k).all() and (c_below[exact] < c_at[exact]).all() and (c_above >= c_at).all() and (c_below[exact] < k).sum() > tab.n // 8
    last = t_at.page(k)[0][exact, k - 1, 3]
    assert np.array_equal(bits(last), bits(t_at.r2[exact])), "the k-th pair lies AT the limit"
    for t, what in ((t_at, "at"), (t_below, "one ulp below"), (t_above, "one ulp above"), (free, "without")):
        check(brute_context, t, k, "radius %s the k-th distance" % what)


# 6. extreme transforms, from host and from device descriptors
def test_extreme_transforms_host_and_device(native_lib):
    import torch
    rng = np.random.default_rng(42)
    tris = soup(rng, 200, edge=0.2)
    M, must_be_inert = extreme_transforms()
    live = live_of(M)
    assert not live[must_be_inert].any() and live.sum() >= 1
    q = queries(np.concatenate([world_hull_points(rng, M[live], tris, 64, 0.2), world_points_near(rng, M[live], tris, 64, 0.01)]))
    free = PairTable(q, M, tris, pair_valid(len(M), len(tris), live))
    tab = free.with_radius(kth_radius(free, 12))
    inst = tab.page(16)[1]
    assert live[inst[inst >= 0]].all() and (inst >= 0).sum() >= 12 * tab.n and (inst < 0).sum() > tab.n
    r = context([tris])
    try:
        info = r.set_instances(M)
        assert info.inert == (~live).sum()
        for k in (4, 16):
            check(r, free, k, "host descriptors", counts=(False,))
            check(r, tab, k, "host descriptors, radius")
        r.set_instances(torch.as_tensor(M, device=torch.device("cuda", 0)))
        check(r, tab, 16, "device descriptors")
    finally:
        r.close()


# 7. objects
@pytest.mark.parametrize("count", (2, 3))
def test_objects(native_lib, count):
    rng = np.random.default_rng(43)
    parts = [arrays(soup(rng, 200, edge=0.2)), arrays(soup(rng, 150, edge=0.2, offset=0.5), soup(rng, 50, edge=0.3)), single_triangle()][:count]
    scene, ranges = concat(parts)
    tris = scene_triangles(scene)
    obj_of_tri = np.concatenate([np.full(n, k) for k, (f, n) in enumerate(triangle_ranges(scene[4], ranges))])
    M = regular_transforms(12)
    objects = np.arange(12) % count
    q = queries(np.concatenate([world_hull_points(rng, M, tris, 96, 0.05), world_points_near(rng, M, tris, 96, 0.02)]))
    q[96:, 3] = 5.0
    whole = PairTable(q, M, tris)
    tab = whole.with_valid(pair_valid(12, len(tris), None, None, None, None, objects, obj_of_tri))
    rec, inst, _ = tab.page(8)
    hit = inst >= 0
    assert hit.sum() > 96 * 8 and (obj_of_tri[bits(rec)[..., 6][hit]] == objects[inst[hit]]).all()
    assert len(np.unique(objects[inst[hit]])) == count, "every object answers somewhere"
    assert not np.array_equal(bits(whole.page(8)[0]), bits(rec))
    r = capi.Renderer(0)
    try:
        r.upload_scene(*scene)
        r.build_bvh()
        r.set_instances(M)
        check(r, whole, 8, "no object table: every instance shows the scene")
        r.set_objects(ranges)
        with pytest.raises(capi.CapError, match="status 3.*cap_instances_set"):
            run(r, q, 8)  # set_objects dropped the instance table
        r.set_instances(M, objects=objects)
        check(r, tab, 8, "%d objects" % count)
        check(r, tab, 3, "%d objects" % count)
    finally:
        r.close()


# 8. masks
def test_instance_mesh_and_call_masks(native_lib):
    rng = np.random.default_rng(44)
    a, b = soup(rng, 150, edge=0.2), soup(rng, 150, edge=0.2)
    tris = np.concatenate([a, b])
    M = regular_transforms(8)
    imasks = np.uint32([0x01, 0x02, 0x04, 0xFF, 0x03, 0x00, 0x01, 0x02])
    q = queries(np.concatenate([world_hull_points(rng, M, tris, 64, 0.05), world_points_near(rng, M, tris, 64, 0.02)]))
    mesh_of_tri = (np.arange(300) >= 150).astype(np.int64)
    free = PairTable(q, M, tris)
    base = free.with_radius(kth_radius(free, 20))

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
        rec, inst, _ = only_b.page(4)
        assert (bits(rec)[..., 6][inst >= 0] >= 150).all() and (inst >= 0).any()
        check(r, only_b, 4, "a mesh with mask 0 is invisible")
        r.set_instance_masks([0x00, 0x00])
        rec, inst, cnt = run(r, q, 4, counts=True)
        assert (inst == -1).all() and all_miss(rec) and (cnt == 0).all()
        with pytest.raises(capi.CapError):
            run(r, q, 4, mask=0x100)
    finally:
        r.close()


# 9. shapes: degenerate points between good ones, the next page, canaries behind all three outputs
@pytest.fixture(scope="module")
def sizes_case(brute_case):
    tris, M, tab = brute_case
    q = tab.q.copy()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for j, (col, value) in enumerate(((0, nan), (1, inf), (2, -inf), (3, np.float32(-1.0)), (3, nan))):
        q[3 + 7 * j::64, col] = value  # degenerate points between good ones
    t = PairTable(q, M, tris)
    assert t.bad.sum() == 20
    first = t.page(3)
    return q, first, t.page(3, cursors_of(first[0], first[1]))


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_sizes_degenerate_points_and_canaries(brute_context, sizes_case, n):
    import torch
    q, first, second = sizes_case
    k = 3
    reps = -(-n // len(q))
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:n]
    dev = torch.device("cuda", 0)
    out = torch.full((n * k + 8, 8), CANARY, dtype=torch.int32, device=dev)
    ins = torch.full((n * k + 8,), CANARY, dtype=torch.int32, device=dev)
    cnt = torch.full((n + 8,), CANARY, dtype=torch.int32, device=dev)
    pts = torch.as_tensor(tile(q), device=dev).contiguous()
    L, r = capi.lib(), brute_context
    torch.cuda.synchronize()
    for flags, want, what in ((0, first, "n = %d" % n), (CONTINUE, second, "n = %d, continued" % n)):
        assert L.cap_closest_instances_multi(r.ctx, pts.data_ptr(), n, k, out.data_ptr(), ins.data_ptr(), cnt.data_ptr(), flags, None) == 0
        r.sync()
        rec, gi, gc = out.view(torch.float32).cpu().numpy(), ins.cpu().numpy(), cnt.cpu().numpy()
        assert_pair_pages((rec[:n * k].reshape(n, k, 8), gi[:n * k].reshape(n, k)), (tile(want[0]), tile(want[1])), what)
        assert_counts(gc[:n], tile(want[2]), what)
        assert (bits(rec[n * k:]) == CANARY).all() and (gi[n * k:].view(np.uint32) == CANARY).all() and (gc[n:].view(np.uint32) == CANARY).all(), \
            "nothing behind the last record, instance or count"
    bad = ~np.isfinite(tile(q)[:, 0:3]).all(1) | ~(tile(q)[:, 3] >= 0)
    assert (bits(rec[:n * k].reshape(n, k, 8)[bad]) == np.uint32([0, 0, 0, 0, 0, 0, MISS, 0])).all() and (gc[:n][bad] == 0).all()


def test_k0_counts_only(brute_case, brute_context):
    _, _, tab = brute_case
    rec, inst, cnt = run(brute_context, tab.q, 0, counts=True)
    assert rec.shape == (tab.n, 0, 8) and inst.shape == (tab.n, 0)
    assert_counts(cnt, tab.counts(), "k = 0")
    with pytest.raises(capi.CapError):
        run(brute_context, tab.q, 0)
    with pytest.raises(capi.CapError):
        run(brute_context, tab.q, 0, counts=True, resume=(rec, inst))


@pytest.mark.parametrize("count", (1, 2, 3, 5))
def test_few_instances_and_a_one_triangle_scene(native_lib, count):
    """1, 2, 3 and 5 instances exercise the top level's padding; the one-triangle scene has a leaf for a root"""
    rng = np.random.default_rng(45)
    M = regular_transforms(6)[1:1 + count]
    for tris in (soup(rng, 100, edge=0.2), soup(rng, 1, edge=0.5)):
        q = queries(np.concatenate([world_hull_points(rng, M, tris, 48, 0.3), world_points_near(rng, M, tris, 48, 0.05)]))
        q[48:, 3] = rng.uniform(0.0, 0.2, 48).astype(np.float32) * np.linalg.norm(M[0, :, :3])
        tab = PairTable(q, M, tris)
        c = tab.counts()
        assert (c[:48] == count * len(tris)).all() and 0 < (c[48:] > 0).sum() < 48
        r = context([tris])
        try:
            assert r.bvh_info().triangle_count == len(tris)
            r.set_instances(M)
            check(r, tab, 4, "%d instances, %d triangles" % (count, len(tris)))
        finally:
            r.close()


# 10. state and arguments
def test_state_refit_rebuild_and_replaced_tables(native_lib):
    rng = np.random.default_rng(46)
    tris = soup(rng, 300, edge=0.2)
    M, M2 = regular_transforms(8), regular_transforms(8, seed=77)
    q = queries(np.concatenate([world_hull_points(rng, M, tris, 64, 0.05), world_points_near(rng, M, tris, 64, 0.02)]))
    P = arrays(tris)[0]
    moved = (P + np.float32([0.05, -0.02, 0.03]) + (rng.random(P.shape) - 0.5).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    tab, tab_moved, tab2 = PairTable(q, M, tris), PairTable(q, M, moved.reshape(-1, 3, 3)), PairTable(q, M2, tris)
    assert not np.array_equal(bits(tab.page(4)[0]), bits(tab_moved.page(4)[0])) and not np.array_equal(bits(tab.page(4)[0]), bits(tab2.page(4)[0]))
    r = context([tris])
    try:
        with pytest.raises(capi.CapError, match="status 3.*cap_instances_set"):
            run(r, q, 4)
        r.set_instances(M)
        check(r, tab, 4, "the first table", counts=(False,))
        r.set_instances(M2)
        check(r, tab2, 4, "a second set_instances replaces the answers", counts=(False,))
        r.set_instances(M)
        r.update_vertices(positions=moved)
        with pytest.raises(capi.CapError, match="status 3.*cap_bvh_refit"):
            run(r, q, 4)
        r.refit_bvh()
        check(r, tab_moved, 4, "after the refit", counts=(False,))
        r.build_bvh()
        check(r, tab_moved, 4, "after a rebuild", counts=(False,))
        r.set_instances(None)
        with pytest.raises(capi.CapError, match="status 3"):
            run(r, q, 4)
    finally:
        r.close()


def test_argument_contract(native_lib, brute_case):
    import torch
    tris, M, tab = brute_case
    dev = torch.device("cuda", 0)
    L = capi.lib()
    n, k = 128, 4
    want = tab.first(n).page(k)
    pts = torch.as_tensor(tab.q[:n], device=dev).contiguous()
    out = torch.full((n * k + 8, 8), CANARY, dtype=torch.int32, device=dev)
    ins = torch.full((n * k + 8,), CANARY, dtype=torch.int32, device=dev)
    cnt = torch.full((n + 8,), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    P, O, I, Cn = pts.data_ptr(), out.data_ptr(), ins.data_ptr(), cnt.data_ptr()
    opts = lambda *o: ctypes.byref(capi.TraceOptions(o[0], o[1], (ctypes.c_uint32 * 2)(*o[2:])))
    r = capi.Renderer(0)
    try:
        call = lambda p=P, m=n, kk=k, o=O, i=I, c=Cn, flags=0, options=None: L.cap_closest_instances_multi(r.ctx, p, m, kk, o, i, c, flags, options)
        bad = lambda *a, **kw: call(*a, **kw) == ERR_INVALID_ARG
        assert call() == ERR_STATE and b"cap_bvh_build" in L.cap_last_error()  # nothing uploaded
        r.upload_scene(*arrays(tris))
        r.build_bvh()
        assert call() == ERR_STATE and b"cap_instances_set" in L.cap_last_error() and call(P, 0) == ERR_STATE  # the state comes before n == 0
        r.set_instances(M)
        assert L.cap_closest_instances_multi(None, P, n, k, O, I, Cn, 0, None) == ERR_INVALID_ARG
        for flags in (0x04, 0x10, 0x20, 0x01, 0x80000000):
            assert bad(options=opts(flags, 0, 0, 0)) and b"ray_flags" in L.cap_last_error()
        assert bad(options=opts(0, 0, 1, 0)) and bad(options=opts(0, 0, 0, 7)) and b"reserved" in L.cap_last_error()
        assert bad(options=opts(0, 0x100, 0, 0)) and bad(options=opts(0, 0xFFFFFFFF, 0, 0))
        assert bad(flags=2) and bad(flags=0x80000000) and b"unknown flags" in L.cap_last_error()
        assert bad(kk=17) and b"CAP_MULTI_MAX_K" in L.cap_last_error()
        assert bad(kk=0) and bad(kk=0, i=None) and bad(kk=0, o=None) and bad(kk=0, o=None, i=None, c=None) and b"k = 0 counts only" in L.cap_last_error()
        assert bad(kk=0, o=None, i=None, flags=CONTINUE) and b"CAP_MULTI_CONTINUE" in L.cap_last_error()
        assert bad(None) and bad(o=None) and bad(i=None) and b"NULL" in L.cap_last_error()
        assert bad(P + 4) and b"points is not 16-byte aligned" in L.cap_last_error()
        assert bad(o=O + 8) and b"output is not 16-byte aligned" in L.cap_last_error()
        assert bad(i=I + 2) and b"instances is not 4-byte aligned" in L.cap_last_error()
        assert bad(c=Cn + 2) and b"counts is not 4-byte aligned" in L.cap_last_error()
        assert bad(o=P) and bad(o=P + 16 * (n - 1)) and b"overlap" in L.cap_last_error()
        assert bad(O + 32 * k * n - 16, o=O) and bad(i=O + 32 * k * n - 4) and bad(i=P) and b"overlap" in L.cap_last_error()
        assert bad(c=I + 4 * k * n - 4) and bad(c=O) and bad(c=P + 16 * n - 4) and bad(i=Cn + 4 * n - 4) and b"overlap" in L.cap_last_error()
        assert bad(P, 1 << 60) and b"address space" in L.cap_last_error()
        assert call(None, 0, k, None, None, None) == 0  # nothing to do
        r.sync()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()) and bool((ins == CANARY).all()) and bool((cnt == CANARY).all()), "nothing is written on an error"
        assert call(options=opts(0, 0, 0, 0)) == 0  # the all-zero options are the plain call
        r.sync()
        rec, gi, gc = out.view(torch.float32).cpu().numpy(), ins.cpu().numpy(), cnt.cpu().numpy()
        assert_pair_pages((rec[:n * k].reshape(n, k, 8), gi[:n * k].reshape(n, k)), want[:2], "the call itself")
        assert_counts(gc[:n], want[2], "the call itself")
        assert (bits(rec[n * k:]) == CANARY).all() and (gi[n * k:].view(np.uint32) == CANARY).all() and (gc[n:].view(np.uint32) == CANARY).all()
        assert call(c=None) == 0 and call(kk=0, o=None, i=None) == 0
        r.sync()
        with pytest.raises(capi.CapError):
            r.closest_instances_multi(torch.zeros((4, 3), device=dev), 4)
        with pytest.raises(capi.CapError):
            r.closest_instances_multi(pts, 17)
        with pytest.raises(capi.CapError):
            r.closest_instances_multi(pts, 4, resume=torch.zeros((n, 4, 8), device=dev))
        with pytest.raises(capi.CapError):
            r.closest_instances_multi(pts, 4, resume=(torch.zeros((n, 4, 8), device=dev), torch.zeros((n, 3), dtype=torch.int32, device=dev)))
    finally:
        r.close()


# 11. render isolation
def test_a_render_is_unchanged_by_a_query_between_its_batches(native_lib, bluenoise, cornell_path):
    geo = capi.Geometry(cornell_path)
    cam = capi.cornell_camera(64, 64)
    rng = np.random.default_rng(5)
    M = np.stack([identity()[0], affine(rotation(rng) * 0.5, (300, 100, -200)), affine(np.diag([1.0, 2.0, 0.5]), (-50, 20, 10))])
    q = queries(rng.random((200, 3)).astype(np.float32) * 700.0 - 100.0, 150.0)
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
                got = r.closest_instances_multi(q, 8, counts=True)
                after = (bits(r.readback(capi.BUF_ACCUM_SUM)), r.stats().as_dict())
                assert np.array_equal(before[0], after[0])
                assert {k: v for k, v in before[1].items() if not k.startswith("ms_")} == {k: v for k, v in after[1].items() if not k.startswith("ms_")}
                P = geo.positions.reshape(-1, 3)
                tris = np.concatenate([P[geo.indices[int(d[3]):int(d[3]) + int(d[2])].astype(np.int64) + int(d[1])].reshape(-1, 3, 3) for d in geo.meshes])
                want = PairTable(q, M, tris).page(8)
                assert_pair_pages(got[:2], want[:2], "the Cornell box under three instances")
                assert_counts(got[2], want[2], "the Cornell box under three instances")
            r.render(2, 2, 2, capi.RENDER_AOV)
            s = r.stats()
            result.append((bits(r.readback(capi.BUF_ACCUM_SUM)), (s.rays_primary, s.rays_extension, s.rays_shadow, s.shaded_vertices, s.frames)))
        finally:
            r.close()
    assert np.array_equal(result[0][0], result[1][0]) and result[0][1] == result[1][1]
