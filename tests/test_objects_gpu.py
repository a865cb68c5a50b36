"""Objects on the GPU (cap_objects_set, cap_objects_info, cap_instances_set_ex): instanced queries over a forest of per-object trees,
every record, instance index and occlusion word raw-compared with the brute force of tests/object_support.py -- per object the
box-free brute force of tests/instance_support.py on the object's own triangles under its own instances, from the W the library read
back, so no tolerance enters a hit comparison."""
import ctypes
import math

import numpy as np
import pytest

from capsaicin_amd import capi
from filter_support import stacked_quads_meshes
from instance_support import (aimed_rays, bits, degenerate_rays, extreme_transforms, f32, grid_scene, random_rays, regular_transforms, rotation,
                              unit_cube)
from instance_support import expected as scene_expected
from object_support import MISS, concat, expected, mesh_of_triangles, object_candidates, scene_triangles, single_triangle, triangle_ranges
from refit_support import Scene, context, cornell_scene

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_STATE = 1, 3
AUTO, LBVH = 0, 1
LEAF_MAX = 2  # triangles per traversal leaf (cap_leaf.h)


def live_of(W):
    return ~np.all(W.reshape(len(W), -1) == 0, axis=1)


def check(r, rays, exp, what, **kw):
    """closest records, instance indices and occlusion words of `rays` against the brute force's, raw uint32 compares, every ray"""
    rec, inst, occ, _ = exp
    hits, gi = r.trace_instances(rays, **kw)
    bad = np.flatnonzero(np.any(bits(hits) != rec, axis=1) | (gi.view(np.uint32) != inst))
    assert len(bad) == 0, "%s: %d of %d closest records differ, first ray %d: got %s inst %d, expected %s inst %d" % (
        what, len(bad), len(rays), bad[0], hits[bad[0]], gi[bad[0]], rec[bad[0]].view(f32), np.int32(inst[bad[0]]))
    kw.pop("first_hit", None)
    got = r.trace_instances_occlusion(rays, **kw)
    bad = np.flatnonzero(got != occ)
    assert len(bad) == 0, "%s: %d of %d occlusion words differ, first ray %d" % (what, len(bad), len(rays), bad[0])


def box_of(tris):
    return tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)


# ---- the scene of tests 1, 3, 4, 5, 6, 9: four objects in one upload ----
N_REGULAR = 72


def four_objects():
    parts = [unit_cube()[0], stacked_quads_meshes(12, 0.25, flip_every=3)[0], single_triangle(), grid_scene(30)[0]]
    arrays, ranges = concat(parts)
    tris, tr = scene_triangles(arrays), triangle_ranges(arrays[4], ranges)
    assert tr.tolist() == [[0, 12], [12, 24], [36, 1], [37, 60]] and ranges[:, 1].tolist() == [6, 12, 1, 1]
    M = np.concatenate([regular_transforms(N_REGULAR), extreme_transforms()[0]])
    masks = np.full(len(M), 0xFF, np.uint32)
    masks[5::11] = 0x0F
    masks[7] = 0
    objects = (np.arange(len(M)) % 4).astype(np.uint32)
    rays = []
    for k, (f, n) in enumerate(tr):  # aimed at every instance's own object
        lo, hi = box_of(tris[f:f + n])
        mine = objects == k
        rays += [aimed_rays(M[mine], lo, hi, 9, seed=9 + k), aimed_rays(M[:N_REGULAR][mine[:N_REGULAR]], lo, hi, 6, seed=19 + k, distances=(1.0,))]
    rays = np.concatenate(rays + [random_rays(900), degenerate_rays()])
    assert len(M) >= 64 and len(rays) >= 2000
    return dict(parts=parts, scene=Scene(*arrays), ranges=ranges, tris=tris, tr=tr, mot=mesh_of_triangles(arrays[4]), M=M, masks=masks, objects=objects,
                rays=rays, exp=None, W=None, cands=None)


@pytest.fixture(scope="module")
def four():
    return four_objects()


def forest_context(s, build=None):
    r = context(s["scene"], build)
    info = r.set_objects(s["ranges"])
    assert info.count == len(s["ranges"]) and info.triangles == int(s["tr"][:, 1].sum()) and info.nodes == int((s["tr"][:, 1] - 1).sum())
    return r


def brute_force(s, W):
    """the brute force of the fixture's table, once: it depends on W alone"""
    if s["exp"] is None:
        live = live_of(W)
        s["cands"] = object_candidates(s["rays"], W, live, s["objects"], s["tris"], s["tr"])
        s["W"], s["exp"] = W, expected(s["rays"], W, live, s["masks"], s["objects"], s["tris"], s["tr"], s["mot"], cands=s["cands"])
    return s["exp"]


# ---- 1. bit-exact against the brute force ----
@pytest.mark.parametrize("build", (AUTO, LBVH))
def test_bit_exact_against_brute_force(native_lib, four, build):
    s = four
    r = forest_context(s, build)
    try:
        info = r.set_instances(s["M"], s["masks"], objects=s["objects"])
        W, _ = r.instances_readback()
        live = live_of(W)
        must_be_inert = np.r_[np.zeros(N_REGULAR, bool), extreme_transforms()[1]]
        assert info.count == len(s["M"]) and info.inert == int((~live).sum())
        assert np.all(live[:N_REGULAR]) and not np.any(live[must_be_inert])
        first = s["exp"] is None
        rec, inst, occ, lists = brute_force(s, W)
        if first:
            n_hit = int((inst != MISS).sum())
            n_multi = sum(1 for h in lists if len({x[3] for x in h}) >= 2)
            objs_hit = sorted({int(s["objects"][i]) for i in inst[inst != MISS]})
            print("%d rays, %d hit, %d occluded, %d with >= 2 instances hit, objects of the closest hits %s" % (len(rec), n_hit, int(occ.sum()), n_multi, objs_hit))
            assert n_hit > len(rec) // 4 and n_multi > 100
            assert objs_hit == [0, 1, 2, 3], "every object is some ray's closest hit"
            assert not np.any(np.isin(inst, np.flatnonzero(~live))), "an inert instance is never hit"
            hit_tri = rec[inst != MISS, 3].astype(np.int64)
            f, n = s["tr"][s["objects"][inst[inst != MISS]]].T
            assert np.all((hit_tri >= f) & (hit_tri < f + n)), "a hit triangle belongs to its instance's object"
        assert np.array_equal(bits(W), bits(s["W"])), "W does not depend on the builder"
        check(r, s["rays"], s["exp"], "four objects, builder %d" % build)
    finally:
        r.close()


# ---- 2. more than eight objects ----
def test_twelve_objects(native_lib):
    cube = unit_cube()[0]
    sizes = 0.25 * 1.3 ** np.arange(12)
    parts = [(cube[0] * f32(sz),) + cube[1:] for sz in sizes]
    arrays, ranges = concat(parts)
    tris, tr = scene_triangles(arrays), triangle_ranges(arrays[4], ranges)
    rng = np.random.default_rng(71)
    n = 120
    M = np.stack([np.c_[rotation(rng) * rng.uniform(0.5, 2.0), rng.uniform(-12, 12, 3)] for _ in range(n)]).astype(f32)
    objects = (np.arange(n) % 12).astype(np.uint32)
    rays = np.concatenate([aimed_rays(M[objects == k], (0, 0, 0), (sizes[k],) * 3, 3, seed=72 + k, distances=(1.0, 100.0)) for k in range(12)]
                          + [random_rays(300, 15.0, seed=73)])
    r = context(Scene(*arrays))
    try:
        assert r.set_objects(ranges).count == 12
        info = r.set_instances(M, objects=objects)
        assert info.inert == 0
        W, _ = r.instances_readback()
        exp = expected(rays, W, live_of(W), None, objects, tris, tr)
        assert (exp[1] != MISS).sum() > len(rays) // 4 and len({int(objects[i]) for i in exp[1][exp[1] != MISS]}) == 12
        check(r, rays, exp, "twelve objects")
    finally:
        r.close()


# ---- 3. a forest tree is the object's own tree ----
@pytest.mark.parametrize("k", range(4))
def test_forest_tree_is_the_objects_own_tree(native_lib, four, k):
    s = four
    mine = s["objects"] == k
    M, masks = s["M"][mine], s["masks"][mine]
    first = int(s["tr"][k, 0])
    a = forest_context(s)
    b = context(Scene(*s["parts"][k]))
    try:
        a.set_instances(M, masks, objects=np.full(len(M), k))
        b.set_instances(M, masks)
        Wa, Ba = a.instances_readback()
        Wb, Bb = b.instances_readback()
        assert np.array_equal(bits(Wa), bits(Wb)) and np.array_equal(bits(Ba), bits(Bb)), "W and world boxes are those of the object uploaded alone"
        ha, ia = a.trace_instances(s["rays"])
        hb, ib = b.trace_instances(s["rays"])
        assert np.array_equal(bits(ha)[:, :3], bits(hb)[:, :3]) and np.array_equal(ia, ib)
        miss = bits(hb)[:, 3] == MISS
        assert np.array_equal(bits(ha)[:, 3] == MISS, miss) and (~miss).sum() > 50
        assert np.array_equal(bits(ha)[~miss, 3], bits(hb)[~miss, 3] + np.uint32(first)), "triangle = local id + first_triangle"
        assert np.array_equal(a.trace_instances_occlusion(s["rays"]), b.trace_instances_occlusion(s["rays"]))
    finally:
        a.close()
        b.close()


# ---- 4. one object covering every mesh equals no object table ----
def test_one_all_covering_object_equals_no_table(native_lib, four):
    s = four
    a = context(s["scene"])
    b = context(s["scene"])
    try:
        info = b.set_objects([[0, len(s["scene"].meshes)]])
        assert info.count == 1 and info.triangles == len(s["tris"])
        a.set_instances(s["M"], s["masks"])
        b.set_instances(s["M"], s["masks"])  # plain cap_instances_set: instances of object 0
        (Wa, Ba), (Wb, Bb) = a.instances_readback(), b.instances_readback()
        assert np.array_equal(bits(Wa), bits(Wb)) and np.array_equal(bits(Ba), bits(Bb))
        (ha, ia), (hb, ib) = a.trace_instances(s["rays"]), b.trace_instances(s["rays"])
        assert np.array_equal(bits(ha), bits(hb)) and np.array_equal(ia, ib) and (ia >= 0).sum() > len(ia) // 4
        assert np.array_equal(a.trace_instances_occlusion(s["rays"]), b.trace_instances_occlusion(s["rays"]))
        b.set_instances(s["M"], s["masks"], objects=np.zeros(len(s["M"])))  # ... and the same through cap_instances_set_ex
        (hc, ic) = b.trace_instances(s["rays"])
        assert np.array_equal(bits(ha), bits(hc)) and np.array_equal(ia, ic)
        a.set_instances(s["M"], s["masks"], objects=np.zeros(len(s["M"])))  # without a table index 0 is the whole scene
        (hd, id_) = a.trace_instances(s["rays"])
        assert np.array_equal(bits(ha), bits(hd)) and np.array_equal(ia, id_)
    finally:
        a.close()
        b.close()


# ---- 5. boxes are the object's, not the scene's ----
def image_box(A, lo, hi):
    """exact (float64) box of the images of the corners of [lo, hi] under the affine map A (3, 4)"""
    c = np.array([[(hi if k >> j & 1 else lo)[j] for j in range(3)] for k in range(8)], np.float64)
    img = c @ A[:, :3].T + A[:, 3]
    return img.min(0), img.max(0)


def boxes_of(s):
    r = forest_context(s)
    try:
        r.set_instances(s["M"], s["masks"], objects=s["objects"])
        W, boxes = r.instances_readback()
        return W, boxes.astype(np.float64)
    finally:
        r.close()


def test_world_boxes_contain_their_object(native_lib, four):
    """every live regular instance's world box contains the image of every vertex of ITS object, and stays within what
    k_instance_setup's own formula pads: the image box of the object's bounds padded by 2e-5 max(1, |coordinate|) (the object box B),
    plus at most pad = c eps (kappa X + |A| |W_t|) + 4 eps X (per axis the kernel takes A's row sum for |A|) with c = 32, kappa <= CAP_INSTANCE_MAX_CONDITION, and the outward rounding to
    float32 (2 ulp of X).  With |A| |W_t| <= kappa |t| <= kappa X: pad <= (2 c kappa + 4) eps X.  The kernel maps the corners with
    A = inverse(fl32(inverse(M))), the test with M: at most 8 kappa eps X apart.  A box from the SCENE's bounds exceeds that for every
    object smaller than the scene."""
    s = four
    W, boxes = boxes_of(s)
    live = live_of(W)
    eps = 2.0 ** -24
    for i in range(N_REGULAR):
        assert live[i]
        f, n = s["tr"][s["objects"][i]]
        P = s["tris"][f:f + n].reshape(-1, 3).astype(np.float64)
        A = s["M"][i].astype(np.float64)
        img = P @ A[:, :3].T + A[:, 3]
        assert np.all(img >= boxes[i, 0]) and np.all(img <= boxes[i, 1]), "world box %d does not contain the image of a vertex of its object" % i
        lo, hi = P.min(0), P.max(0)
        pad_o = 2e-5 * np.maximum(1.0, np.maximum(np.abs(lo), np.abs(hi)))
        ilo, ihi = image_box(A, lo - pad_o, hi + pad_o)
        Wd = W[i].astype(np.float64)
        kappa = np.abs(np.linalg.inv(Wd[:, :3])).sum(1).max() * np.abs(Wd[:, :3]).sum(1).max()
        X = np.abs(boxes[i]).max()
        slack = ((2 * 32 + 8) * kappa + 4 + 4) * eps * X + 1e-6 * (ihi - ilo)
        assert np.all(boxes[i, 0] >= ilo - slack) and np.all(boxes[i, 1] <= ihi + slack), "world box %d is larger than its object's padded image" % i
    assert np.all(np.isinf(boxes[~live])), "an inert instance has an empty box"


def test_world_boxes_are_tight_around_their_object(native_lib, four):
    """Each half-extent of a live regular instance's world box is at most that of the exact image box of its object's bounds, times
    1 + 1e-3, plus 1e-4 max|coordinate| of the box.
    From k_instance_setup: stored half-extent on axis r = h'_r + pad_r (+ 1 ulp), h'_r the half-extent of the image of the object box B
    (the bounds padded by 2e-5 max(1, |c|): at most 1 + 4e-5 / extent times the bounds' image) and
    pad_r = 32 eps (kappa_r X + |A_r| |W_t|) + 4 eps X <= (64 kappa_r + 4) eps X, |A_r| the row sum of A = inverse(W), kappa_r = |A_r| |W|.
    1e-4 X covers that outright while kappa_r <= 26; beyond, the relative part takes over, because the image's half-extent on axis r
    grows with the same |A_r| (h_r >= |A_r| times the object's smallest half-extent): an axis with a large kappa_r is a long one.
    The kernel's formula evaluated in float64 on the host for this table uses at most 0.48 of the margin (instance 34, kappa 33).
    A box from the scene's bounds, or one padded on every axis with the largest row sum, does not fit (1.14 at instance 9)."""
    s = four
    W, boxes = boxes_of(s)
    worst = []
    for i in range(N_REGULAR):
        f, n = s["tr"][s["objects"][i]]
        P = s["tris"][f:f + n].reshape(-1, 3).astype(np.float64)
        ilo, ihi = image_box(s["M"][i].astype(np.float64), P.min(0), P.max(0))
        h, got = (ihi - ilo) / 2, (boxes[i, 1] - boxes[i, 0]) / 2
        allowed = h * (1 + 1e-3) + 1e-4 * np.abs(boxes[i]).max()
        Wd = W[i].astype(np.float64)
        kappa = np.abs(np.linalg.inv(Wd[:, :3])).sum(1).max() * np.abs(Wd[:, :3]).sum(1).max()
        worst.append((((got - h) / (allowed - h)).max(), i, int(s["objects"][i]), kappa))
    worst.sort(reverse=True)
    print("used fraction of the margin (instance, object, kappa): " + ", ".join("%.2f (%d, %d, %.0f)" % w for w in worst[:6]))
    over = [w for w in worst if w[0] > 1.0]
    assert not over, "%d of %d boxes exceed the margin, worst %.2f x at instance %d (object %d, kappa %.0f)" % ((len(over), N_REGULAR) + over[0])


# ---- 6. cap_objects_info ----
@pytest.mark.parametrize("build", (AUTO, LBVH))
def test_objects_info(native_lib, four, build):
    s = four
    r = forest_context(s, build)
    try:
        info = r.objects_info()
        assert len(info) == 4
        for k, o in enumerate(info):
            f, n = (int(x) for x in s["tr"][k])
            P = s["tris"][f:f + n].reshape(-1, 3)
            assert (o["first_triangle"], o["triangle_count"], o["node_count"]) == (f, n, n - 1)
            assert np.array_equal(o["bounds_lo"], P.min(0)) and np.array_equal(o["bounds_hi"], P.max(0))
            assert o["max_depth"] >= math.ceil(math.log2(math.ceil(n / LEAF_MAX))) and o["max_depth"] <= 64
            assert o["builder"] == capi.Renderer.BVH_BUILD_LBVH and o["reserved"] == 0  # AUTO takes the Morton hierarchy up to 64 triangles
        assert info["max_depth"][2] == 0, "a one-triangle object has no node"
        n = ctypes.c_uint32(99)
        one = np.zeros(1, capi.OBJECT_INFO_DTYPE)
        assert capi.lib().cap_objects_info(r.ctx, one.ctypes.data, 1, ctypes.byref(n)) == 0 and n.value == 4 and one[0].tobytes() == info[0].tobytes()
        r.set_objects(None)
        assert len(r.objects_info()) == 0
    finally:
        r.close()


def test_objects_take_the_builder_of_their_size(native_lib):
    """AUTO: the Morton hierarchy up to 64 triangles, the clustering above (the surface-area builder from 4 096 on); by name: the mode,
    the host builder mapped to its device counterpart.  Every tree against the brute force."""
    parts = [unit_cube()[0], grid_scene(100, seed=81)[0], grid_scene(40, seed=82)[0]]  # 12, 200, 80 triangles
    arrays, ranges = concat(parts)
    tris, tr = scene_triangles(arrays), triangle_ranges(arrays[4], ranges)
    M = regular_transforms(18, seed=83, spread=6.0)
    objects = (np.arange(18) % 3).astype(np.uint32)
    rays = np.concatenate([aimed_rays(M[objects == k], *box_of(tris[f:f + n]), 6, seed=84 + k, distances=(1.0, 100.0)) for k, (f, n) in enumerate(tr)]
                          + [random_rays(200, 10.0, seed=85)])
    R = capi.Renderer
    want = {R.BVH_BUILD_AUTO: [R.BVH_BUILD_LBVH, R.BVH_BUILD_PLOC, R.BVH_BUILD_PLOC], R.BVH_BUILD_LBVH: [R.BVH_BUILD_LBVH] * 3,
            R.BVH_BUILD_SAH: [R.BVH_BUILD_SAH_DEVICE] * 3, R.BVH_BUILD_PLOC: [R.BVH_BUILD_PLOC] * 3, R.BVH_BUILD_SAH_DEVICE: [R.BVH_BUILD_SAH_DEVICE] * 3}
    exp = None
    for mode, builders in want.items():
        r = context(Scene(*arrays), mode)
        try:
            r.set_objects(ranges)
            info = r.objects_info()
            assert info["builder"].tolist() == builders, mode
            assert np.all(info["max_depth"] >= [math.ceil(math.log2(math.ceil(n / LEAF_MAX))) for n in tr[:, 1]]) and np.all(info["max_depth"] <= 64)
            r.set_instances(M, objects=objects)
            if exp is None:
                W, _ = r.instances_readback()
                exp = expected(rays, W, live_of(W), None, objects, tris, tr)
                assert (exp[1] != MISS).sum() > len(rays) // 4
            check(r, rays, exp, "build mode %d" % mode)
        finally:
            r.close()


# ---- the small scene of tests 7 and 8 ----
@pytest.fixture(scope="module")
def small():
    parts = [unit_cube()[0], stacked_quads_meshes(6, 0.25, flip_every=3)[0], single_triangle()]
    arrays, ranges = concat(parts)
    tris, tr = scene_triangles(arrays), triangle_ranges(arrays[4], ranges)
    M = regular_transforms(24, seed=41, spread=4.0).astype(f32)
    objects = (np.arange(24) % 3).astype(np.uint32)
    rays = np.concatenate([aimed_rays(M[objects == k], *box_of(tris[f:f + n]), 5, seed=42 + k, distances=(1.0, 100.0)) for k, (f, n) in enumerate(tr)]
                          + [random_rays(100, 6.0, seed=43)])
    return dict(scene=Scene(*arrays), ranges=ranges, tris=tris, tr=tr, M=M, objects=objects, rays=rays)


# ---- 7. life cycle and errors ----
def test_life_cycle_and_errors(native_lib, small):
    import torch
    s = small
    scene, rays, M, objects = s["scene"], s["rays"], s["M"], s["objects"]
    dev = torch.device("cuda", 0)
    L = capi.lib()
    rng_ = np.ascontiguousarray(s["ranges"], np.uint32)
    r = capi.Renderer(0)
    try:
        r.upload_scene(scene.positions, scene.normals, scene.texcoords, scene.indices, scene.meshes)
        assert L.cap_objects_set(r.ctx, rng_.ctypes.data, len(rng_), None) == ERR_STATE, "before cap_bvh_build"
        r.build_bvh()
        rt = torch.as_tensor(rays, device=dev)
        out = torch.empty((len(rays), 4), device=dev)
        torch.cuda.synchronize()
        d = np.zeros(len(M), capi.INSTANCE_DESC_DTYPE)
        d["transform"], d["mask"] = M.reshape(-1, 12), 0xFF
        one = np.ones(len(M), np.uint32)
        # without an object table: every host index must be 0
        assert L.cap_instances_set_ex(r.ctx, d.ctypes.data, one.ctypes.data, len(M), 0, None) == ERR_INVALID_ARG
        assert L.cap_trace_instances(r.ctx, rt.data_ptr(), len(rays), out.data_ptr(), None, None) == ERR_STATE, "nothing was installed"
        r.set_objects(s["ranges"])
        r.set_instances(M, objects=objects)
        W, _ = r.instances_readback()
        exp = expected(rays, W, live_of(W), None, objects, s["tris"], s["tr"])
        assert (exp[1] != MISS).sum() > len(rays) // 4
        check(r, rays, exp, "the table")

        def bad(ranges, count=None):
            a = np.ascontiguousarray(ranges, np.uint32).reshape(-1, 2)
            return L.cap_objects_set(r.ctx, a.ctypes.data, len(a) if count is None else count, None)

        n_mesh = len(scene.meshes)
        assert bad([[0, 6], [5, 3]]) == ERR_INVALID_ARG and b"overlap" in L.cap_last_error()
        assert bad([[6, 6], [0, 7]]) == ERR_INVALID_ARG, "overlap, given in the other order"
        assert bad([[0, 6], [6, n_mesh - 5]]) == ERR_INVALID_ARG, "a range past the mesh count"
        assert bad([[n_mesh, 1]]) == ERR_INVALID_ARG
        assert bad([[0, 6], [6, 0]]) == ERR_INVALID_ARG, "mesh_count = 0"
        assert bad(np.zeros((capi.OBJECT_MAX_COUNT + 1, 2)), capi.OBJECT_MAX_COUNT + 1) == ERR_INVALID_ARG
        assert L.cap_objects_set(r.ctx, None, 2, None) == ERR_INVALID_ARG
        big = objects.copy()
        big[3] = 3
        assert L.cap_instances_set_ex(r.ctx, d.ctypes.data, big.ctypes.data, len(M), 0, None) == ERR_INVALID_ARG, "a host object index out of range"
        check(r, rays, exp, "after the rejected calls: nothing changed")
        assert len(r.objects_info()) == 3
        # device descriptors and indices: an out-of-range index makes the instance inert, and it is counted
        info = r.set_instances(torch.as_tensor(M, device=dev), objects=torch.as_tensor(big.astype(np.int32), device=dev))
        Wd, Bd = r.instances_readback()
        assert info.inert == 1 and not live_of(Wd)[3] and live_of(Wd).sum() == len(M) - 1 and np.all(np.isinf(Bd[3]))
        check(r, rays, expected(rays, Wd, live_of(Wd), None, objects, s["tris"], s["tr"]), "device table with one inert instance")
        info = r.set_instances(torch.as_tensor(M, device=dev), objects=torch.as_tensor(objects.astype(np.int32), device=dev))
        assert info.inert == 0
        check(r, rays, exp, "device descriptors and indices")
        # stale trees
        r.update_vertices(scene.positions)
        assert L.cap_objects_set(r.ctx, rng_.ctypes.data, len(rng_), None) == ERR_STATE, "while stale"
        r.refit_bvh()
        check(r, rays, exp, "after a refit of the same vertices")
        # a new object table drops the instance table
        r.set_objects(s["ranges"][::-1])
        assert L.cap_trace_instances(r.ctx, rt.data_ptr(), len(rays), out.data_ptr(), None, None) == ERR_STATE
        assert L.cap_instances_readback(r.ctx, None, None) == ERR_STATE
        r.set_instances(M, objects=2 - objects)  # the same objects under their new indices
        check(r, rays, exp, "ranges in the other order")
        # count = 0 restores the plain behaviour (and drops the instance table as well)
        r.set_objects(None)
        assert L.cap_trace_instances(r.ctx, rt.data_ptr(), len(rays), out.data_ptr(), None, None) == ERR_STATE
        r.set_instances(M)
        W2, _ = r.instances_readback()
        check(r, rays, scene_expected(rays, W2, live_of(W2), None, s["tris"]), "whole-scene instances after the table was removed")
        # cap_scene_upload drops both tables
        r.set_objects(s["ranges"])
        r.set_instances(M, objects=objects)
        r.upload_scene(scene.positions, scene.normals, scene.texcoords, scene.indices, scene.meshes)
        r.build_bvh()
        assert len(r.objects_info()) == 0
        assert L.cap_trace_instances(r.ctx, rt.data_ptr(), len(rays), out.data_ptr(), None, None) == ERR_STATE
        assert L.cap_instances_set_ex(r.ctx, d.ctypes.data, one.ctypes.data, len(M), 0, None) == ERR_INVALID_ARG, "no object table any more"
    finally:
        r.close()


# ---- 8. animated object ----
def test_animated_object(native_lib, small):
    s = small
    scene, rays, M, objects = s["scene"], s["rays"], s["M"], s["objects"]
    r = context(scene)
    try:
        r.set_objects(s["ranges"])
        r.set_instances(M, objects=objects)
        W, B0 = r.instances_readback()
        before = r.objects_info()
        # object 1 (the quads) grows and moves outside its old bounds; the others stay
        P = scene.positions.copy()
        m0, m1 = int(s["ranges"][1, 0]), int(s["ranges"][1, 0] + s["ranges"][1, 1])
        v0, v1 = int(scene.meshes[m0, 1]), int(scene.meshes[m1 - 1, 1] + scene.meshes[m1 - 1, 0])
        P[v0:v1] = P[v0:v1] * f32([2.0, 1.5, 1.0]) + f32([0.5, -0.25, 1.0])
        moved = scene.moved(P).triangles()
        r.update_vertices(P)
        r.refit_bvh()
        W2, B2 = r.instances_readback()
        assert np.array_equal(bits(W2), bits(W))
        changed = np.any(bits(B2) != bits(B0), axis=(1, 2))
        assert np.array_equal(changed, objects == 1), "the boxes of the moved object's instances follow, the others stay"
        after = r.objects_info()
        f, n = s["tr"][1]
        assert np.array_equal(after["bounds_lo"][1], moved[f:f + n].reshape(-1, 3).min(0)) and np.array_equal(after["bounds_hi"][1], moved[f:f + n].reshape(-1, 3).max(0))
        assert after[0].tobytes() == before[0].tobytes() and after[2].tobytes() == before[2].tobytes()
        # aimed at the moved object's new place as well
        lo, hi = box_of(moved[f:f + n])
        rays2 = np.concatenate([rays, aimed_rays(M[objects == 1], lo, hi, 5, seed=47, distances=(1.0, 100.0))])
        exp = expected(rays2, W2, live_of(W2), None, objects, moved, s["tr"])
        old = expected(rays2, W2, live_of(W2), None, objects, s["tris"], s["tr"])
        assert np.any(exp[0] != old[0]), "the rays see the move"
        check(r, rays2, exp, "after the refit")
        r.build_bvh()
        assert r.objects_info().tobytes() == after.tobytes()
        check(r, rays2, exp, "after a rebuild")
    finally:
        r.close()


# ---- 9. filters ----
def test_filters(native_lib, four):
    s = four
    r = forest_context(s)
    try:
        r.set_instances(s["M"], s["masks"], objects=s["objects"])
        W, _ = r.instances_readback()
        brute_force(s, W)
        live = live_of(W)
        sel = np.arange(0, len(s["rays"]), 4)  # a quarter of test 1's rays: the brute force runs once per case
        rays = s["rays"][sel]
        cands = [[c[j] for j in sel] for c in s["cands"]]
        mesh_masks = (1 << (np.arange(len(s["scene"].meshes)) % 8)).astype(np.uint8)
        half = s["masks"].copy()
        half[::2] = 0x55
        cases = [(s["masks"], None, "back", None), (s["masks"], None, "front", 0x0F), (half, mesh_masks, None, None), (half, mesh_masks, "back", 0x33)]
        for im, mm, cull, mask in cases:
            r.set_instances(s["M"], im, objects=s["objects"])
            r.set_instance_masks(mm)
            what = "mesh masks %s cull %s mask %s" % (mm is not None, cull, mask)
            exp = expected(rays, W, live, im, s["objects"], s["tris"], s["tr"], s["mot"], mm, cull, mask, cands)
            assert (exp[1] != MISS).sum() > 20 and np.any(exp[0] != s["exp"][0][sel]), "the filter keeps some hits and changes some records"
            check(r, rays, exp, what, cull=cull, mask=mask)
            # ACCEPT_FIRST_HIT: some member of the set, a miss exactly when it is empty
            hits, gi = r.trace_instances(rays, cull=cull, mask=mask, first_hit=True)
            for k, h in enumerate(exp[3]):
                got = (bits(hits[k])[0], bits(hits[k])[1], bits(hits[k])[2], int(np.uint32(gi[k])), int(bits(hits[k])[3]))
                if not h:
                    assert got[3] == MISS and got[4] == MISS and hits[k, 0] == rays[k, 7], (what, k)
                else:
                    assert got in {(bits(t)[0], bits(u)[0], bits(v)[0], i, g) for t, u, v, i, g in h}, (what, k)
    finally:
        r.close()


# ---- 10. nothing else moved ----
def cornell_frame(r, with_queries=None):
    w = h = 64
    r.set_resolution(w, h)
    r.set_camera(capi.cornell_camera(w, h))
    r.render(0, 2, 2, capi.RENDER_AOV)
    q = with_queries() if with_queries else None
    r.render(2, 2, 2, capi.RENDER_AOV)
    r.sync()
    return bits(r.readback(capi.BUF_ACCUM_SUM)), bits(r.readback(capi.BUF_GBUFFER_GEO)), q


def test_nothing_else_moved(native_lib, bluenoise, cornell_path):
    import torch
    scene, materials = cornell_scene(cornell_path)
    tris = scene.triangles()
    n_mesh = len(scene.meshes)
    ranges = np.array([[n_mesh // 2, n_mesh - n_mesh // 2], [0, n_mesh // 2]], np.uint32)
    tr = triangle_ranges(scene.meshes, ranges)
    rng = np.random.default_rng(61)
    o = rng.uniform(0.1, 0.9, (500, 3)) * (tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)) + tris.reshape(-1, 3).min(0)
    rays = np.c_[o, np.zeros(500), rng.normal(size=(500, 3)), np.full(500, np.inf)].astype(f32)
    M = regular_transforms(40, seed=62, spread=2.0)
    objects = (np.arange(40) % 2).astype(np.uint32)
    dev = torch.device("cuda", 0)

    def run(table):
        r = context(scene, bluenoise=bluenoise)
        try:
            rt = torch.as_tensor(rays, device=dev)
            torch.cuda.synchronize()
            if table:
                r.set_objects(ranges)
                r.set_instances(M, objects=objects)
            frame = cornell_frame(r, (lambda: (r.trace_instances(rt, sync=False), r.trace_instances_occlusion(rt, sync=False))) if table else None)
            plain = (bits(r.trace_rays(rays)), r.trace_occlusion(rays), bits(r.trace_rays_multi(rays, 4)), bits(r.trace_rays(rays, cull="back")))
            if table:
                (h, i), occ = frame[2]
                W, _ = r.instances_readback()
                exp = expected(rays, W, live_of(W), None, objects, tris, tr)
                assert np.array_equal(bits(h.cpu().numpy()), exp[0]) and np.array_equal(i.cpu().numpy().view(np.uint32), exp[1])
                assert np.array_equal(occ.cpu().numpy(), exp[2]) and (exp[1] != MISS).sum() > 100
            return frame[:2], plain
        finally:
            r.close()

    (fa, pa), (fb, pb) = run(True), run(False)
    for x, y in zip(fa + pa, fb + pb):
        assert np.array_equal(x, y), "a call that does not read the object table changed with one installed"
