"""Every traversal-stack size class of the queries on the MI355X, on small deep trees.  A binary-tree walk keeps its stack in LDS, is
compiled once per stack size and is launched by the tree's depth; a push beyond the stack is dropped silently, so a class too small
for its depth answers wrongly for a few rays and nothing faults.  The spiral of tests/deep_tree_support.py gives the host SAH builder a
tree of depth n - 2: n = 18, 19, 26, 27, 34, 35, 40 put a tree on both sides of 16 | 17, 24 | 25 and 32 | 33 and one at 38, and
tests/test_deep_trees.py shows without a GPU that the query sets fill the stacks of these trees up to the last entry and fetch answers
from it.  Here every query family runs on them -- and a render, which reaches the render path's 64-entry kernels without a scene of
millions of triangles -- and every record is compared bit for bit with the box-free brute force of the support modules."""
import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import assert_records, closest
from deep_tree_support import SIZES, depth_of, mesh_masks, point_set, point_walk, ray_set, ray_walk, scales, spiral, spiral_arrays, tri_boxes
from filter_support import MISS, bits, closest_record, faced_hits, filtered_hits, filtered_occlusion, mesh_of_triangles
from instance_multi_support import expected_pages as instance_pages
from instance_support import expected as instance_expected
from instance_support import f32, rotation
from multi_hit_support import hit_list_array, page_to_exhaustion
from object_support import concat, scene_triangles, triangle_ranges
from object_support import expected as object_expected
from refit_support import Scene, context
from test_ray_query_filter_gpu import check_filtered

pytestmark = pytest.mark.gpu
R = capi.Renderer
SAH = R.BVH_BUILD_SAH
SENTINEL = 0x7FBADBAD
KS = (1, 4, 8, 16)
FILTERS = (("back", None), ("front", None), (None, 0x01), (None, 0x80), (None, 0x55), ("back", 0x55))  # (cull, inclusion mask)
_CASES = {}


def scene_class(depth):
    return 32 if depth <= 32 else 64


def instance_class(depth):
    return 24 if depth <= 24 else 32 if depth <= 32 else 64


def point_class(depth):
    return 16 if depth <= 16 else 24 if depth <= 24 else 32 if depth <= 32 else 64


class Case:
    """the spiral of n triangles, its query sets and their brute force, each made once and left unchanged"""

    def __init__(self, n):
        self.n, self.tris = n, spiral(n)
        self.scene = Scene(*spiral_arrays(self.tris))
        self.mot = mesh_of_triangles(self.scene.meshes)
        self.masks = mesh_masks(n)
        self.rays, self.points = ray_set(n), point_set(n)
        self._faced = self._closest = None
        self._filtered, self._occ = {}, {}

    @property
    def faced(self):
        if self._faced is None:
            self._faced = [faced_hits(x, self.tris) for x in self.rays]
        return self._faced

    def lists(self, cull=None, mask=None):
        """per ray the hits that pass (cull, mask) under the mask table, in (t, id) order"""
        if (cull, mask) not in self._filtered:
            self._filtered[cull, mask] = [filtered_hits(x, self.tris, self.mot, self.masks, cull, mask, faced=f) for x, f in zip(self.rays, self.faced)]
        return self._filtered[cull, mask]

    def occlusion(self, cull=None, mask=None):
        if (cull, mask) not in self._occ:
            self._occ[cull, mask] = np.array([filtered_occlusion(x, self.tris, self.mot, self.masks, cull, mask) for x in self.rays], np.int32)
        return self._occ[cull, mask]

    @property
    def closest(self):
        if self._closest is None:
            self._closest = closest(self.points, self.tris)
        return self._closest


def case(n):
    if n not in _CASES:
        _CASES[n] = Case(n)
    return _CASES[n]


def sah_context(c, bluenoise=None):
    r = context(c.scene, SAH, bluenoise)
    info = r.bvh_info()
    assert info.max_depth == depth_of(c.n) and info.stack_entries == scene_class(info.max_depth)
    return r


def traced_with_sentinel(r, rays, any_hit):
    """the records of trace_rays / trace_occlusion written into the head of a longer buffer: the words behind them stay as they were"""
    import torch
    n, pad = len(rays), 64
    if any_hit:
        big = torch.full((n + pad,), SENTINEL, dtype=torch.int32, device="cuda:0")
        got = r.trace_occlusion(rays, out=big[:n])
    else:
        big = torch.full((n + pad, 4), SENTINEL, dtype=torch.int32, device="cuda:0").view(torch.float32)
        got = r.trace_rays(rays, out=big[:n])
    tail = big[n:].cpu().numpy().view(np.uint32)
    assert np.all(tail == SENTINEL), "a query wrote behind its last record"
    return got


# ---- 1. the tree under test is the one the CPU conditions hold for ----
@pytest.mark.parametrize("n", SIZES)
def test_tree_under_test(native_lib, n):
    c = case(n)
    r = sah_context(c)
    try:
        nodes, leaves = r.bvh_readback()
        want_nodes, order, depth = capi.host_sah_build(*tri_boxes(c.tris))
        assert depth == depth_of(n) == r.bvh_info().max_depth
        assert np.array_equal(bits(nodes), bits(want_nodes)) and np.array_equal(leaves, order), "the device holds the host builder's tree"
        # ... so the model walks of tests/test_deep_trees.py are walks of this tree
        _, table = c.closest
        ray_high = max(ray_walk(nodes, leaves, c.tris, x)[0] for x in c.rays[:48])
        point_high = max(point_walk(nodes, leaves, c.tris, q, table[i])[0] for i, q in enumerate(c.points[:24]))
        wide_nodes, wide_depth, wide_top = r.bvh_wide_info()
        print("spiral n %d: host SAH depth %d, stack class %d, model high-water rays %d points %d, wide view %d nodes depth %d top %d" % (
            n, depth, r.bvh_info().stack_entries, ray_high, point_high, wide_nodes, wide_depth, wide_top))
        assert min(ray_high, point_high) >= depth - (2 if n == 40 else 1)
    finally:
        r.close()


# ---- 2. cap_trace_rays / cap_trace_occlusion, wide view on and off ----
@pytest.mark.parametrize("n", SIZES)
def test_trace_rays_and_occlusion(native_lib, n):
    c = case(n)
    lists = c.lists()
    assert max(len(h) for h in lists) > 16
    want = np.stack([closest_record(h, x[7]) for x, h in zip(c.rays, lists)])
    occ = c.occlusion()
    r = sah_context(c)
    try:
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            assert r.debug_get(R.DEBUG_WIDE_IN_USE) == 1 - no_wide
            got = traced_with_sentinel(r, c.rays, False)
            bad = np.nonzero((bits(got) != bits(want)).any(1))[0]
            assert len(bad) == 0, "no_wide8 %d: %d rays differ, first %d: got %s want %s" % (no_wide, len(bad), bad[0], bits(got[bad[0]]), bits(want[bad[0]]))
            got = traced_with_sentinel(r, c.rays, True)
            assert np.array_equal(got, occ), "no_wide8 %d occlusion: rays %s differ" % (no_wide, np.nonzero(got != occ)[0][:8])
    finally:
        r.close()


# ---- 3. the _ex calls: culls, first hit, inclusion masks ----
@pytest.mark.parametrize("n", SIZES)
def test_ex_calls(native_lib, n):
    c = case(n)
    r = sah_context(c)
    try:
        r.set_instance_masks(c.masks)
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            for cull, mask in FILTERS:
                what = "n %d no_wide8 %d cull %s mask %s" % (n, no_wide, cull, mask)
                lists = c.lists(cull, mask)
                check_filtered(r, c.rays, lists, c.occlusion(cull, mask), cull, mask, ks=(), what=what)
                first = r.trace_rays(c.rays, cull=cull, mask=mask, first_hit=True)
                for i, h in enumerate(lists):
                    recs = bits(hit_list_array(h)) if h else bits(closest_record([], c.rays[i, 7]))[None]
                    assert (recs == bits(first[i])).all(1).any(), "%s: the first hit of ray %d is not among its %d hits" % (what, i, len(h))
    finally:
        r.close()


# ---- 4. cap_trace_rays_multi(_ex): every K bucket, counts, paging ----
@pytest.mark.parametrize("n", SIZES)
def test_trace_rays_multi(native_lib, n):
    c = case(n)
    r = sah_context(c)
    try:
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            r.set_instance_masks(None)
            lists = c.lists()
            check_filtered(r, c.rays, lists, None, None, None, ks=KS, what="n %d no_wide8 %d plain" % (n, no_wide))
            walked, pages = page_to_exhaustion(r, c.rays, 4)
            assert len(pages) > 5  # more than 16 hits on some ray: past every page size
            for i, h in enumerate(lists):
                assert np.array_equal(bits(walked[i]), bits(hit_list_array(h))), "no_wide8 %d paging, ray %d" % (no_wide, i)
            r.set_instance_masks(c.masks)
            check_filtered(r, c.rays, c.lists("back", 0x55), None, "back", 0x55, ks=KS, paging=(4,), what="n %d no_wide8 %d back 0x55" % (n, no_wide))
    finally:
        r.close()


# ---- 5. instances of the scene tree ----
def instance_table(seed=3):
    """identity, a rotation with a non-uniform scale, a mirror, an inert one, and two that overlap the first"""
    rng = np.random.default_rng(seed)
    eye = np.c_[np.eye(3), np.zeros(3)]
    M = [eye,
         np.c_[rotation(rng) @ np.diag([0.5, 1.0, 2.0]), [0.3, -0.2, 0.1]],
         np.c_[rotation(rng) @ np.diag([-1.0, 1.0, 1.0]), [-0.1, 0.2, 0.3]],
         np.zeros((3, 4)),
         np.c_[np.eye(3), [0.05, 0.0, -0.05]],
         np.c_[rotation(rng), [0.0, 0.1, 0.0]]]
    return np.array(M, f32), np.array([0xFF, 0xFF, 0x0F, 0xFF, 0xF0, 0xFF], np.uint32)


def instance_rays(c, count=72):
    """a part of the ray set (random, axis-aligned, from outside, from the centroids) and the degenerate rays: the instances' offsets are
    of the middle triangles' size, so the identity instance sees the whole chain around a ray and the others its larger half"""
    pick = np.r_[0:24, 48:60, 72:84, 96:96 + c.n:3]
    rays = c.rays[pick][:count].copy()
    return np.concatenate([rays, c.rays[-7:]])


def compare_instances(out, exp, counts, what):
    rec, inst, cnt = exp
    h, gi = np.asarray(out[0]), np.asarray(out[1])
    assert h.shape == rec.shape and gi.shape == inst.shape, (what, h.shape, gi.shape)
    bad = np.flatnonzero(np.any(bits(h).reshape(len(rec), -1) != rec.reshape(len(rec), -1), axis=1) | np.any(gi.view(np.uint32) != inst, axis=1))
    assert len(bad) == 0, "%s: %d of %d pages differ, first ray %d: got %s inst %s expected %s inst %s" % (
        what, len(bad), len(rec), bad[0], h[bad[0]], gi[bad[0]], rec[bad[0]].view(f32), inst[bad[0]].view(np.int32))
    if counts:
        assert np.array_equal(np.asarray(out[2]).view(np.uint32), cnt), "%s: counts differ" % what


def check_instances(r, rays, exp, what, ks=KS, **kw):
    """closest, occlusion, first hit, and the pages of every K bucket with and without counts, against one brute force"""
    rec, inst, occ, lists = exp
    h, gi = r.trace_instances(rays, **kw)
    bad = np.flatnonzero((bits(h) != rec).any(1) | (gi.view(np.uint32) != inst))
    assert len(bad) == 0, "%s closest: %d rays differ, first %d: got %s %d want %s %d" % (what, len(bad), bad[0], bits(h[bad[0]]), gi[bad[0]], rec[bad[0]], inst[bad[0]])
    assert np.array_equal(r.trace_instances_occlusion(rays, **kw), occ), "%s occlusion" % what
    h, gi = r.trace_instances(rays, first_hit=True, **kw)
    for j, hits in enumerate(lists):
        if not hits:
            assert np.array_equal(bits(h[j]), rec[j]) and gi[j] == -1, "%s first hit: ray %d has no hit" % (what, j)
            continue
        members = {(int(bits(t)[0]), int(bits(u)[0]), int(bits(v)[0]), int(g), int(i)) for t, u, v, i, g in hits}
        assert tuple(int(w) for w in bits(h[j])) + (int(gi[j]),) in members, "%s: the first hit of ray %d is not among its %d hits" % (what, j, len(hits))
    for k in ks:
        pages = instance_pages(lists, rays, k)
        for counts in (False, True):
            compare_instances(r.trace_instances_multi(rays, k, counts=counts, **kw), pages, counts, "%s k %d counts %s" % (what, k, counts))
    compare_instances(r.trace_instances_multi(rays, 0, counts=True, **kw), instance_pages(lists, rays, 0), True, "%s counts only" % what)


@pytest.mark.parametrize("n", SIZES)
def test_instances(native_lib, n):
    c = case(n)
    M, inst_masks = instance_table()
    rays = instance_rays(c)
    r = sah_context(c)
    try:
        r.set_instance_masks(c.masks)
        info = r.set_instances(M, inst_masks)
        W, _ = r.instances_readback()
        live = ~np.all(W.reshape(len(W), -1) == 0, axis=1)
        assert info.count == 6 and info.inert == 1 and live.tolist() == [True, True, True, False, True, True]
        print("spiral n %d: instanced walks take the %d-entry class" % (n, instance_class(depth_of(n))))
        plain = instance_expected(rays, W, live, inst_masks, c.tris, c.mot, c.masks)
        longest, several = max(len(h) for h in plain[3]), sum(1 for h in plain[3] if len({x[3] for x in h}) >= 2)
        assert longest > 16 and several > len(rays) // 4, (longest, several)
        check_instances(r, rays, plain, "n %d instances" % n)
        check_instances(r, rays, instance_expected(rays, W, live, inst_masks, c.tris, c.mot, c.masks, "back", 0x55), "n %d instances back 0x55" % n,
                        ks=(4, 16), cull="back", mask=0x55)
    finally:
        r.close()


# ---- 6. cap_closest_points, with and without a mesh-mask table ----
@pytest.mark.parametrize("n", SIZES)
def test_closest_points(native_lib, n):
    c = case(n)
    want, _ = c.closest
    r = sah_context(c)
    try:
        print("spiral n %d: closest-point walks take the %d-entry class" % (n, point_class(depth_of(n))))
        assert_records(r.closest_points(c.points), want, "n %d" % n)
        r.set_instance_masks(c.masks)
        assert_records(r.closest_points(c.points), want, "n %d, a table and every mask bit" % n)
        for mask in (0x01, 0x55, 0x80):
            passes = (c.masks[c.mot] & mask) != 0
            assert_records(r.closest_points(c.points, mask=mask), closest(c.points, c.tris, passes)[0], "n %d mask 0x%02x" % (n, mask))
        # instances installed: the instanced calls go by their own depth source, the point query keeps the scene's
        r.set_instances(instance_table()[0])
        assert_records(r.closest_points(c.points, mask=0x55), closest(c.points, c.tris, (c.masks[c.mot] & 0x55) != 0)[0], "n %d after set_instances" % n)
    finally:
        r.close()


# ---- 7. objects: the instance kernels on the objects' depth ----
@pytest.mark.parametrize("n", SIZES)
def test_objects(native_lib, n):
    c = case(n)
    half = spiral_arrays(c.tris[:n // 2])
    arrays, ranges = concat([spiral_arrays(c.tris), half])  # (object ranges may not overlap: the first half is uploaded once more)
    tris, tr = scene_triangles(arrays), triangle_ranges(arrays[4], ranges)
    assert tr.tolist() == [[0, n], [n, n // 2]]
    mot = mesh_of_triangles(arrays[4])
    M, inst_masks = instance_table()
    objects = np.array([0, 1, 0, 1, 1, 0], np.uint32)
    rays = instance_rays(c, 48)
    r = context(Scene(*arrays), SAH)
    try:
        info = r.set_objects(ranges)
        per = r.objects_info()
        assert info.count == 2 and per["triangle_count"].tolist() == [n, n // 2]
        print("spiral n %d: scene tree depth %d; object trees (device builders %s) depth %s, forest max_depth %d" % (
            n, r.bvh_info().max_depth, per["builder"].tolist(), per["max_depth"].tolist(), info.max_depth))
        assert info.max_depth == per["max_depth"].max() <= 64
        r.set_instances(M, inst_masks, objects=objects)
        W, _ = r.instances_readback()
        live = ~np.all(W.reshape(len(W), -1) == 0, axis=1)
        exp = object_expected(rays, W, live, inst_masks, objects, tris, tr, mot)
        assert max(len(h) for h in exp[3]) > 16
        check_instances(r, rays, exp, "n %d objects" % n, ks=(1, 16))
    finally:
        r.close()


# ---- 8. the device builders on the same scene: parity, whatever depth they reach ----
@pytest.mark.parametrize("build", (R.BVH_BUILD_LBVH, R.BVH_BUILD_PLOC, R.BVH_BUILD_SAH_DEVICE, R.BVH_BUILD_AUTO))
def test_other_builders(native_lib, build):
    c = case(40)
    r = context(c.scene, build)
    try:
        info = r.bvh_info()
        print("spiral n 40, builder %d: depth %d, stack class %d, wide view depth %d" % (build, info.max_depth, info.stack_entries, r.bvh_wide_info()[1]))
        assert info.max_depth <= 64 and info.stack_entries == scene_class(info.max_depth)
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            check_filtered(r, c.rays, c.lists(), c.occlusion(), None, None, ks=KS, paging=(4,), what="builder %d no_wide8 %d" % (build, no_wide))
        assert_records(r.closest_points(c.points), c.closest[0], "builder %d" % build)
    finally:
        r.close()


# ---- 9. refit: the same tree over moved vertices ----
def test_refit(native_lib):
    n = 35
    c = case(n)
    P = c.scene.positions.astype(np.float64)
    s_mid = float(np.abs(c.tris[n // 2]).max())
    moved = (P * (1.0 + 0.2 * np.tanh(P[:, [1, 2, 0]] / s_mid)) * [1.1, 0.9, 1.25]).astype(f32)  # a smooth stretch, different per axis
    tris = moved.reshape(-1, 3, 3)
    r = sah_context(c)
    try:
        before = r.bvh_readback()
        r.update_vertices(positions=moved)
        r.refit_bvh()
        info = r.bvh_info()
        assert info.max_depth == depth_of(n) and info.stack_entries == 64
        nodes, leaves = r.bvh_readback()
        assert np.array_equal(leaves, before[1]) and np.array_equal(bits(nodes[:, 12:16]), bits(before[0][:, 12:16])), "a refit keeps the topology"
        assert not np.array_equal(bits(nodes[:, 0:12]), bits(before[0][:, 0:12]))
        lists = [[h[:4] for h in faced_hits(x, tris)] for x in c.rays]
        occ = np.array([filtered_occlusion(x, tris, c.mot, None) for x in c.rays], np.int32)
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            check_filtered(r, c.rays, lists, occ, None, None, ks=(1, 16), paging=(4,), what="refit no_wide8 %d" % no_wide)
        assert_records(r.closest_points(c.points), closest(c.points, tris)[0], "refit")
        M, inst_masks = instance_table()
        r.set_instances(M, inst_masks)
        W, _ = r.instances_readback()
        live = ~np.all(W.reshape(len(W), -1) == 0, axis=1)
        rays = instance_rays(c, 48)
        check_instances(r, rays, instance_expected(rays, W, live, inst_masks, tris), "refit instances", ks=(4, 16))
    finally:
        r.close()


# ---- 10. the render path's tree kernels on a 64-entry tree ----
@pytest.mark.parametrize("n", (35, 40))
def test_render(native_lib, bluenoise, n):
    from oracle import cap_oracle as O
    c = case(n)
    w, h, bounces = 64, 48, 3
    # Primary rays end at t = 1e6 (camera.h:59-60), short of the largest triangles: the camera stands at 3 s_k from the origin for the
    # largest s_k with 4 s_k < 1e6 and looks at the origin down the triangles' common normal -- the middle rays pass through every box
    # of the chain -- and the bounces reach the triangles beyond.
    s = scales(n)
    far = 3.0 * s[4.0 * s < 1.0e6].max() / np.sqrt(3.0)
    cam = capi.camera_from_config({"position": [far, far, far], "forward": [-1.0, -1.0, -1.0], "focal_length": 0.02, "sensor_x": 0.036}, w, h)
    sc = O.Scene(c.scene.positions, c.scene.normals, c.scene.texcoords, c.scene.indices, c.scene.meshes)
    ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1], cam.focal_length)
    ref = [sc.render_frame(ocam, bluenoise, w, h, f, bounces, threads=4) for f in (0, 1)]
    geo = ref[0]["gbuffer_geo"].view(np.uint32)
    assert (geo[..., 3] != MISS).mean() > 0.25 and len(np.unique(geo[..., 2])) >= 4, "the camera sees several triangles of the chain"
    assert ref[0]["rays"][1] > 0 and ref[0]["rays"][2] > 0
    r = sah_context(c, bluenoise)
    try:
        assert r.bvh_info().stack_entries == 64
        r.set_resolution(w, h)
        r.set_camera(cam)
        r.set_traversal(1)
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            assert r.debug_get(R.DEBUG_WIDE_IN_USE) == 1 - no_wide  # 0: k_trace_closest_refill<64>, k_trace_any<64>
            for f in (0, 1):
                r.stats_reset()
                r.render(f, 1, bounces, capi.RENDER_AOV)
                r.sync()
                s = r.stats()
                for name, kind in (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("direct", capi.BUF_DIRECT), ("indirect", capi.BUF_INDIRECT),
                                   ("normal_depth", capi.BUF_NORMAL_DEPTH)):
                    assert np.array_equal(bits(r.readback(kind)), bits(ref[f][name])), "n %d no_wide8 %d frame %d: plane %s differs" % (n, no_wide, f, name)
                assert (s.rays_primary, s.rays_extension, s.rays_shadow) == ref[f]["rays"], "n %d no_wide8 %d frame %d" % (n, no_wide, f)
    finally:
        r.close()
