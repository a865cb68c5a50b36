"""Closest-point queries over instances on the GPU (cap_closest_instances): every record compared bit for bit, all eight words plus the
instance, with the numpy float32 brute force of closest_instances_support.py over every (instance, triangle)."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_instances_support import (MISS, affine, assert_pairs, bits, closest_instances, flat_record, identity, instance_box_points, live_of,
                                       near_translations, pair_valid, world_hull_points, world_points_near)
from closest_point_support import arrays, assert_records, context, queries, soup, sphere
from instance_support import extreme_transforms, flatten, grid_scene, regular_transforms, rotation, translations
from multi_hit_support import stacked_quads
from object_support import concat, scene_triangles, single_triangle, triangle_ranges

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 3
CANARY = 0x7FC0BEEF  # a NaN pattern no record holds
B = capi.Renderer  # the CapBvhBuild values


def run(r, q, mask=None):
    return r.closest_instances(np.ascontiguousarray(q, np.float32), mask=mask)


def with_tight_radius(q, want):
    """the queries again with the radius a hair above the answer's distance: the bound starts thin instead of becoming so"""
    q2 = q.copy()
    q2[:, 3] = np.sqrt(want[0][:, 3]) * np.float32(1.000001)
    return q2


# 1. ties
def tie_points(n_quads, dz):
    z_mid = (np.arange(n_quads - 1) + 0.5) * dz
    out = []
    for z in z_mid[::3]:
        out += [(0.5, 0.25, z), (0.25, 0.5, z), (0.5, 0.5, z), (0.25, 0.25, z), (0.75, 0.75, z), (0, 0, z), (1, 1, z), (1, 0, z), (0, 1, z), (2, 2, z), (-1, 0.5, z)]
    out += [(0.5, 0.5, -3.0), (40.0, -30.0, 100.0), (0.5, 0.25, n_quads * dz + 5.0), (0.25, 0.25, 0.0), (1.0, 1.0, dz)]
    return queries(out)


def test_ties_go_to_the_lower_instance_then_the_lower_id(native_lib):
    _, tris = stacked_quads(40, 0.25)
    M = np.stack([identity()[0], identity()[0], identity()[0], affine(np.eye(3), (0, 0, 0.25))])
    q = tie_points(40, 0.25)
    rec, inst, table = closest_instances(q, M, tris, with_table=True)
    tied = table == rec[:, 3][:, None, None]
    assert (inst >= 0).all() and (tied.sum((1, 2)) >= 2).sum() >= 0.9 * len(q), "the expected set really holds ties"
    assert (tied[:, 0].any(1) & tied[:, 3].any(1)).sum() > 10, "... and ties across instances with different transforms"
    assert (inst == 0).sum() > 0.9 * len(q)
    r = context([tris])
    try:
        r.set_instances(M)
        assert_pairs(run(r, q), (rec, inst), "ties")
    finally:
        r.close()


# 2. the brute force, under three builders
@pytest.fixture(scope="module")
def brute_case():
    """a 600-triangle soup under 32 transforms, 256 points uniform in the instances' boxes (half of them in the box of them all) and
    256 near world surfaces, the second half with radii around the answers' distances; the brute force, once"""
    rng = np.random.default_rng(21)
    tris = soup(rng, 600, edge=0.1)
    M = regular_transforms(32)
    q = queries(np.concatenate([world_hull_points(rng, M, tris, 128, 0.05), instance_box_points(rng, M, tris, 128), world_points_near(rng, M, tris, 256, 0.02)]))
    free = closest_instances(q[256:], M, tris)
    q[256:, 3] = np.sqrt(free[0][:, 3]) * rng.uniform(0.5, 1.5, 256).astype(np.float32)
    return tris, M, q, closest_instances(q, M, tris)


@pytest.mark.parametrize("build", (B.BVH_BUILD_LBVH, B.BVH_BUILD_SAH, B.BVH_BUILD_SAH_DEVICE), ids=("lbvh", "sah", "sah_device"))
def test_every_builder_equals_the_brute_force(native_lib, brute_case, build):
    tris, M, q, want = brute_case
    inst = want[1]
    assert len(np.unique(inst[inst >= 0])) >= 16 and len(np.unique(inst[:256])) >= 16, "the winners lie in many instances"
    assert (inst[:256] >= 0).all() and 50 < (inst[256:] >= 0).sum() < 206, "the radii split the second half into hits and misses"
    r = context([tris], build)
    try:
        info = r.set_instances(M)
        assert info.inert == 0
        assert_pairs(run(r, q), want, "builder %d" % build)
    finally:
        r.close()


# 3. extreme transforms, from host and from device descriptors
def test_extreme_transforms_host_and_device(native_lib):
    import torch
    rng = np.random.default_rng(22)
    tris = soup(rng, 200, edge=0.2)
    M, must_be_inert = extreme_transforms()
    live = live_of(M)
    assert not live[must_be_inert].any() and live.sum() >= 1
    q = queries(np.concatenate([world_hull_points(rng, M[live], tris, 128, 0.2), world_points_near(rng, M[live], tris, 128, 0.01)]))
    want = closest_instances(q, M, tris, pair_valid(len(M), len(tris), live))
    assert (want[1] >= 0).all() and live[want[1]].all()
    r = context([tris])
    try:
        info = r.set_instances(M)
        assert info.inert == (~live).sum(), "the debug entry decides as the device does"
        assert_pairs(run(r, q), want, "host descriptors")
        r.set_instances(torch.as_tensor(M, device=torch.device("cuda", 0)))
        assert_pairs(run(r, q), want, "device descriptors")
    finally:
        r.close()


# 4. scenes built against the prune
def prune_scene(name):
    rng = np.random.default_rng(23)
    tris = soup(rng, 600, edge=0.1)
    if name == "translations near 4096":
        M = near_translations(regular_transforms(16))
        pts = np.concatenate([world_hull_points(rng, M, tris, 128, 0.05), world_points_near(rng, M, tris, 128, 0.01)])
    elif name == "sphere from the image of its centre":
        tris = sphere()
        R = rotation(rng)
        c = np.float64([3, -2, 5])
        M = np.stack([affine(R @ np.diag([1.0, 30.0, 90.0]) @ R.T, c)])
        pts = (c + np.concatenate([np.zeros((1, 3)), rng.normal(size=(383, 3)) * 1e-3, rng.normal(size=(128, 3)) * 1e-6])).astype(np.float32)
    elif name == "points 1e5 away":
        M = regular_transforms(16)
        d = rng.normal(size=(128, 3))
        pts = (d / np.linalg.norm(d, axis=1, keepdims=True) * 1e5).astype(np.float32)
    elif name == "16 instances at one place":
        tris = soup(rng, 300, edge=0.2)
        R = rotation(rng)
        M = np.stack([affine(R @ _small_rotation(rng), (5, 6, 7)) for k in range(16)])
        pts = np.concatenate([world_hull_points(rng, M, tris, 64, -0.25), world_hull_points(rng, M, tris, 64, 0.3), world_points_near(rng, M, tris, 128, 0.01)])
    else:
        raise KeyError(name)
    return tris, M, queries(pts)


def _small_rotation(rng):
    a = rng.normal(size=3) * 0.02
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Q, _ = np.linalg.qr(np.eye(3) + K)
    return Q * np.sign(np.diag(Q))[None]


@pytest.mark.parametrize("name", ("translations near 4096", "sphere from the image of its centre", "points 1e5 away", "16 instances at one place"))
def test_scenes_against_the_prune(native_lib, name):
    tris, M, q = prune_scene(name)
    want = closest_instances(q, M, tris)
    assert (want[1] >= 0).all()
    q2 = with_tight_radius(q, want)
    want2 = closest_instances(q2, M, tris)
    assert (want2[1] >= 0).sum() > 0.9 * len(q)
    r = context([tris])
    try:
        info = r.set_instances(M)
        assert info.inert == 0
        if name == "16 instances at one place":
            _, boxes = r.instances_readback()
            p = q[:64, 0:3]  # (the middle of the hull)
            inside = ((p[:, None] >= boxes[None, :, 0]) & (p[:, None] <= boxes[None, :, 1])).all(2)
            assert inside.all(1).sum() > 40, "points that every world box holds"
        assert_pairs(run(r, q), want, name)
        assert_pairs(run(r, q2), want2, name + ", tight radius")
    finally:
        r.close()


# 5. the three identities, on the device
def test_identities_on_the_device(native_lib):
    rng = np.random.default_rng(24)
    scene, tris = grid_scene(30)
    T = len(tris)
    tr = np.float32([[0, 0, 0], [16, 0, 0], [0, 0, 0], [-32, 16, 48], [64, -64, 16], [16, 0, 0], [-64, 64, -64]])  # coinciding copies
    q = queries(rng.integers(-100 * 16, 100 * 16 + 1, (512, 3)) / 16.0)
    q[256:, 3] = 24.0
    r = capi.Renderer(0)
    flat = capi.Renderer(0)
    try:
        r.upload_scene(*scene)
        r.build_bvh()
        # 1. one identity instance is the flat query
        r.set_instances(identity())
        rec, inst = run(r, q)
        plain = r.closest_points(q)
        assert_records(rec, plain, "identity instance against cap_closest_points")
        assert ((inst == 0) == (bits(plain)[:, 6] != MISS)).all() and ((inst == -1) | (inst == 0)).all()
        # 2. translations on the grid are the flattened scene
        r.set_instances(translations(tr))
        rec, inst = run(r, q)
        flat.upload_scene(*flatten(scene, tr))
        flat.build_bvh()
        got_flat = flat.closest_points(q)
        assert_records(flat_record(rec, inst, T), got_flat, "translations against the flattened scene")
        assert len(np.unique(inst)) >= 5 and (inst == 2).sum() == 0 and (inst == 5).sum() == 0 and (inst == -1).sum() > 0
        assert_pairs((rec, inst), closest_instances(q, translations(tr), tris), "translations against the brute force")
        # 3. everything scaled by a power of two
        M = regular_transforms(8)
        qs = queries(world_hull_points(rng, M, tris, 256, 0.05), 16.0)
        r.set_instances(M)
        rec, inst = run(r, qs)
        assert 0 < (inst >= 0).sum() < len(qs)
        for k in (3, -2):
            s = np.float32(2.0 ** k)
            r.set_instances(M * s)
            rec_s, inst_s = run(r, qs * s)
            assert np.array_equal(inst_s, inst) and np.array_equal(bits(rec_s)[:, 4:8], bits(rec)[:, 4:8])
            assert np.array_equal(bits(rec_s[:, 0:3]), bits(rec[:, 0:3] * s)) and np.array_equal(bits(rec_s[:, 3]), bits(rec[:, 3] * s * s))
    finally:
        r.close()
        flat.close()


# 6. objects
@pytest.mark.parametrize("count", (2, 3))
def test_objects(native_lib, count):
    rng = np.random.default_rng(25)
    parts = [arrays(soup(rng, 200, edge=0.2)), arrays(soup(rng, 150, edge=0.2, offset=0.5), soup(rng, 50, edge=0.3)), single_triangle()][:count]
    scene, ranges = concat(parts)
    tris = scene_triangles(scene)
    tr = triangle_ranges(scene[4], ranges)
    obj_of_tri = np.concatenate([np.full(n, k) for k, (f, n) in enumerate(tr)])
    M = regular_transforms(12)
    objects = np.arange(12) % count
    q = queries(np.concatenate([world_hull_points(rng, M, tris, 192, 0.05), world_points_near(rng, M, tris, 192, 0.02)]))
    q[192:, 3] = 5.0
    want = closest_instances(q, M, tris, pair_valid(12, len(tris), None, None, None, None, objects, obj_of_tri))
    hit = want[1] >= 0
    assert hit.sum() > 192 and (obj_of_tri[bits(want[0])[hit, 6]] == objects[want[1][hit]]).all()
    assert len(np.unique(objects[want[1][hit]])) == count, "every object answers somewhere"
    whole = closest_instances(q, M, tris)
    assert not np.array_equal(bits(whole[0]), bits(want[0])), "the whole scene under every instance answers differently"
    r = capi.Renderer(0)
    try:
        r.upload_scene(*scene)
        r.build_bvh()
        r.set_instances(M)
        assert_pairs(run(r, q), whole, "no object table: every instance shows the scene")
        r.set_objects(ranges)
        with pytest.raises(capi.CapError, match="status 3.*cap_instances_set"):
            run(r, q)  # set_objects dropped the instance table
        r.set_instances(M, objects=objects)
        assert_pairs(run(r, q), want, "%d objects" % count)
    finally:
        r.close()


# 7. masks
def test_masks_and_option_errors(native_lib):
    import torch
    rng = np.random.default_rng(26)
    a, b = soup(rng, 150, edge=0.2), soup(rng, 150, edge=0.2)
    tris = np.concatenate([a, b])
    M = regular_transforms(8)
    imasks = np.uint32([0x01, 0x02, 0x04, 0xFF, 0x03, 0x00, 0x01, 0x02])
    q = queries(np.concatenate([world_hull_points(rng, M, tris, 128, 0.05), world_points_near(rng, M, tris, 128, 0.02)]))
    mesh_of_tri = (np.arange(300) >= 150).astype(np.int64)

    def ref(inst_masks=None, mesh_masks=None, mask=None):
        tm = None if mesh_masks is None else np.uint32(mesh_masks)[mesh_of_tri]
        return closest_instances(q, M, tris, pair_valid(8, 300, None, inst_masks, tm, mask))

    dev = torch.device("cuda", 0)
    r = context([a, b])
    try:
        r.set_instances(M, masks=imasks)
        want = ref(imasks)
        assert (want[1] != 5).all() and not np.array_equal(bits(want[0]), bits(ref()[0]))
        assert_pairs(run(r, q), want, "instance masks")
        assert_pairs(run(r, q, mask=0x01), ref(imasks, None, 0x01), "instance masks and the call's mask")
        assert_pairs(run(r, q, mask=0x08), ref(imasks, None, 0x08), "a call mask only 0xFF passes")
        r.set_instance_masks([0x05, 0x02])
        assert_pairs(run(r, q), ref(imasks, [0x05, 0x02]), "instance and mesh masks")
        assert_pairs(run(r, q, mask=0x06), ref(imasks, [0x05, 0x02], 0x06), "instance, mesh and call masks")
        r.set_instance_masks([0x00, 0xFF])
        only_b = ref(imasks, [0x00, 0xFF])
        assert (bits(only_b[0])[only_b[1] >= 0, 6] >= 150).all()
        assert_pairs(run(r, q), only_b, "a mesh with mask 0 is invisible")
        r.set_instance_masks([0x00, 0x00])
        none = run(r, q)
        assert (none[1] == -1).all() and (bits(none[0])[:, 6] == MISS).all() and np.isinf(none[0][:, 3]).all()
        r.set_instance_masks(None)
        r.set_instances(M, masks=np.zeros(8, np.uint32))
        none = run(r, q)
        assert (none[1] == -1).all() and (bits(none[0])[:, 6] == MISS).all(), "mask 0 on every instance: all misses"
        r.set_instances(M, masks=imasks)

        # options the call refuses: nothing is written
        L = capi.lib()
        pts = torch.as_tensor(q, device=dev).contiguous()
        out = torch.full((len(q), 8), CANARY, dtype=torch.int32, device=dev)
        ins = torch.full((len(q),), CANARY, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        call = lambda *o: L.cap_closest_instances(r.ctx, pts.data_ptr(), len(q), out.data_ptr(), ins.data_ptr(),
                                                  ctypes.byref(capi.TraceOptions(o[0], o[1], (ctypes.c_uint32 * 2)(*o[2:]))))
        for flags in (0x04, 0x10, 0x20, 0x01, 0x80000000):
            assert call(flags, 0, 0, 0) == ERR_INVALID_ARG and b"ray_flags" in L.cap_last_error()
        assert call(0, 0, 1, 0) == ERR_INVALID_ARG and call(0, 0, 0, 7) == ERR_INVALID_ARG and b"reserved" in L.cap_last_error()
        assert call(0, 0x100, 0, 0) == ERR_INVALID_ARG and call(0, 0xFFFFFFFF, 0, 0) == ERR_INVALID_ARG
        r.sync()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()) and bool((ins == CANARY).all())
        assert call(0, 0, 0, 0) == 0  # the all-zero options are the plain call
        r.sync()
        assert_pairs((out.view(torch.float32).cpu().numpy(), ins.cpu().numpy()), want, "all-zero options")
        with pytest.raises(capi.CapError):
            r.closest_instances(q, mask=0x100)
    finally:
        r.close()


# 8. shapes
@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_sizes_with_canaries(native_lib, brute_case, n):
    import torch
    tris, M, q, want = brute_case
    q = q.copy()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for k, (col, value) in enumerate(((0, nan), (1, inf), (2, -inf), (3, np.float32(-1.0)), (3, nan))):
        q[3 + 7 * k::64, col] = value  # degenerate points between good ones
    bad = ~np.isfinite(q[:, 0:3]).all(1) | ~(q[:, 3] >= 0)
    rec, inst = want[0].copy(), want[1].copy()
    rec[bad] = 0
    rec.view(np.uint32)[bad, 6] = MISS
    inst[bad] = -1
    assert bad.sum() == 40
    reps = -(-n // len(q))
    qn, wn, wi = np.tile(q, (reps, 1))[:n], np.tile(rec, (reps, 1))[:n], np.tile(inst, reps)[:n]
    dev = torch.device("cuda", 0)
    out = torch.full((n + 8, 8), CANARY, dtype=torch.int32, device=dev)
    ins = torch.full((n + 8,), CANARY, dtype=torch.int32, device=dev)
    pts = torch.as_tensor(qn, device=dev).contiguous()
    L = capi.lib()
    r = context([tris])
    try:
        r.set_instances(M)
        torch.cuda.synchronize()
        assert L.cap_closest_instances(r.ctx, pts.data_ptr(), n, out.data_ptr(), ins.data_ptr(), None) == 0
        r.sync()
        got, gi = out.view(torch.float32).cpu().numpy(), ins.cpu().numpy()
        assert_pairs((got[:n], gi[:n]), (wn, wi), "n = %d" % n)
        assert (bits(got[n:]) == CANARY).all() and (gi[n:].view(np.uint32) == CANARY).all(), "nothing behind the last record or instance"
        # device_instances = NULL
        out2 = torch.full((n + 8, 8), CANARY, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert L.cap_closest_instances(r.ctx, pts.data_ptr(), n, out2.data_ptr(), None, None) == 0
        r.sync()
        assert bool((out2 == out).all())
    finally:
        r.close()


@pytest.mark.parametrize("count", (1, 2, 3, 5))
def test_few_instances_and_a_one_triangle_scene(native_lib, count):
    """1, 2, 3 and 5 instances exercise the top level's padding; the one-triangle scene has a leaf for a root"""
    rng = np.random.default_rng(27)
    M = regular_transforms(6)[1:1 + count]
    for tris in (soup(rng, 100, edge=0.2), soup(rng, 1, edge=0.5)):
        q = queries(np.concatenate([world_hull_points(rng, M, tris, 96, 0.3), world_points_near(rng, M, tris, 96, 0.05)]))
        q[96:, 3] = rng.uniform(0.0, 0.2, 96).astype(np.float32) * np.linalg.norm(M[0, :, :3])
        want = closest_instances(q, M, tris)
        assert (want[1][:96] >= 0).all() and 0 < (want[1][96:] >= 0).sum() < 96
        r = context([tris])
        try:
            assert r.bvh_info().triangle_count == len(tris)
            r.set_instances(M)
            assert_pairs(run(r, q), want, "%d instances, %d triangles" % (count, len(tris)))
        finally:
            r.close()


# 9. state and arguments
def test_state_refit_rebuild_and_replaced_tables(native_lib):
    rng = np.random.default_rng(28)
    tris = soup(rng, 300, edge=0.2)
    M, M2 = regular_transforms(8), regular_transforms(8, seed=77)
    q = queries(np.concatenate([world_hull_points(rng, M, tris, 128, 0.05), world_points_near(rng, M, tris, 128, 0.02)]))
    P = arrays(tris)[0]
    moved = (P + np.float32([0.05, -0.02, 0.03]) + (rng.random(P.shape) - 0.5).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    want, want_moved, want2 = closest_instances(q, M, tris), closest_instances(q, M, moved.reshape(-1, 3, 3)), closest_instances(q, M2, tris)
    assert not np.array_equal(bits(want[0]), bits(want_moved[0])) and not np.array_equal(bits(want[0]), bits(want2[0]))
    r = context([tris])
    try:
        with pytest.raises(capi.CapError, match="status 3.*cap_instances_set"):
            run(r, q)
        r.set_instances(M)
        assert_pairs(run(r, q), want, "the first table")
        r.set_instances(M2)
        assert_pairs(run(r, q), want2, "a second set_instances replaces the answers")
        r.set_instances(M)
        r.update_vertices(positions=moved)
        with pytest.raises(capi.CapError, match="status 3.*cap_bvh_refit"):
            run(r, q)
        r.refit_bvh()
        assert_pairs(run(r, q), want_moved, "after the refit")
        r.build_bvh()
        assert_pairs(run(r, q), want_moved, "after a rebuild")
        r.set_instances(None)
        with pytest.raises(capi.CapError, match="status 3"):
            run(r, q)
    finally:
        r.close()


def test_argument_contract(native_lib, brute_case):
    import torch
    tris, M, q, want = brute_case
    dev = torch.device("cuda", 0)
    L = capi.lib()
    n = 128
    pts = torch.as_tensor(q[:n], device=dev).contiguous()
    out = torch.full((n + 8, 8), CANARY, dtype=torch.int32, device=dev)
    ins = torch.full((n + 8,), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    P, O, I = pts.data_ptr(), out.data_ptr(), ins.data_ptr()
    r = capi.Renderer(0)
    try:
        call = lambda p=P, m=n, o=O, i=I: L.cap_closest_instances(r.ctx, p, m, o, i, None)
        assert call() == ERR_STATE and b"cap_bvh_build" in L.cap_last_error()  # nothing uploaded
        r.upload_scene(*arrays(tris))
        r.build_bvh()
        assert call() == ERR_STATE and b"cap_instances_set" in L.cap_last_error() and call(P, 0) == ERR_STATE  # the state comes before n == 0
        r.set_instances(M)
        assert L.cap_closest_instances(None, P, n, O, I, None) == ERR_INVALID_ARG
        assert call(None) == ERR_INVALID_ARG and call(P, n, None) == ERR_INVALID_ARG and b"NULL" in L.cap_last_error()
        assert call(P + 4) == ERR_INVALID_ARG and b"points is not 16-byte aligned" in L.cap_last_error()
        assert call(P, n, O + 8) == ERR_INVALID_ARG and b"output is not 16-byte aligned" in L.cap_last_error()
        assert call(P, n, O, I + 2) == ERR_INVALID_ARG and b"instances is not 4-byte aligned" in L.cap_last_error()
        assert call(P, n, P) == ERR_INVALID_ARG and call(P, n, P + 16 * (n - 1)) == ERR_INVALID_ARG and b"overlap" in L.cap_last_error()
        assert call(O + 32 * (n - 1), n, O) == ERR_INVALID_ARG
        assert call(P, n, O, O + 32 * n - 4) == ERR_INVALID_ARG and call(P, n, O, P) == ERR_INVALID_ARG and b"overlap" in L.cap_last_error()
        assert call(P, 1 << 60) == ERR_INVALID_ARG and b"address space" in L.cap_last_error()
        assert call(None, 0, None, None) == 0  # nothing to do
        r.sync()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()) and bool((ins == CANARY).all()), "nothing is written on an error"
        assert call() == 0
        r.sync()
        got, gi = out.view(torch.float32).cpu().numpy(), ins.cpu().numpy()
        assert_pairs((got[:n], gi[:n]), (want[0][:n], want[1][:n]), "the call itself")
        assert (bits(got[n:]) == CANARY).all() and (gi[n:].view(np.uint32) == CANARY).all()
        with pytest.raises(capi.CapError):
            r.closest_instances(torch.zeros((4, 3), device=dev))
        with pytest.raises(capi.CapError):
            r.closest_instances(pts, out=torch.zeros((n, 4), device=dev))
    finally:
        r.close()


# 10. render isolation
def test_a_render_is_unchanged_by_a_query_between_its_batches(native_lib, bluenoise, cornell_path):
    geo = capi.Geometry(cornell_path)
    cam = capi.cornell_camera(64, 64)
    rng = np.random.default_rng(5)
    M = np.stack([identity()[0], affine(rotation(rng) * 0.5, (300, 100, -200)), affine(np.diag([1.0, 2.0, 0.5]), (-50, 20, 10))])
    q = queries(rng.random((500, 3)).astype(np.float32) * 700.0 - 100.0)
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
                got = r.closest_instances(q)
                after = (bits(r.readback(capi.BUF_ACCUM_SUM)), r.stats().as_dict())
                assert np.array_equal(before[0], after[0])
                assert {k: v for k, v in before[1].items() if not k.startswith("ms_")} == {k: v for k, v in after[1].items() if not k.startswith("ms_")}
                P = geo.positions.reshape(-1, 3)
                tris = np.concatenate([P[geo.indices[int(d[3]):int(d[3]) + int(d[2])].astype(np.int64) + int(d[1])].reshape(-1, 3, 3) for d in geo.meshes])
                assert_pairs(got, closest_instances(q, M, tris), "the Cornell box under three instances")
            r.render(2, 2, 2, capi.RENDER_AOV)
            s = r.stats()
            result.append((bits(r.readback(capi.BUF_ACCUM_SUM)), (s.rays_primary, s.rays_extension, s.rays_shadow, s.shaded_vertices, s.frames)))
        finally:
            r.close()
    assert np.array_equal(result[0][0], result[1][0]) and result[0][1] == result[1][1]
