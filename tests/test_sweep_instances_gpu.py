"""Sphere sweep queries over instances on the GPU (cap_sweep_instances): every record compared bit for bit, all eight words plus the
instance, with the numpy float32 brute force of sweep_instances_support.py over every (instance, triangle)."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_instances_support import triangles_of
from closest_point_support import arrays, assert_records, context, needles, queries, soup, sphere
from instance_support import extreme_transforms, flatten, grid_scene, regular_transforms, rotation, translations
from multi_hit_support import stacked_quads
from object_support import concat, scene_triangles, single_triangle, triangle_ranges
from sweep_instances_support import (MISS, affine, aimed_sweeps, assert_pairs, bits, expected, flat_record, identity, live_of, near_translations,
                                     pair_valid, sweep_instances)
from sweep_support import sweep_queries, sweep_scene
from test_sweep_instances import ROT90, known_cases
from test_sweep_spheres import TRI, degenerate_sweeps

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 3
CANARY = 0x7FC0BEEF  # a NaN pattern no record holds
B = capi.Renderer  # the CapBvhBuild values
f32 = np.float32
RADII = (0.01, 0.03, 0.1)  # of the instance's size


def run(r, q, mask=None):
    return r.sweep_instances(np.ascontiguousarray(q, f32), mask=mask)


def check(tris, M, q, what, build=None, valid=None):
    want = expected(q, M, tris, valid)
    r = context([tris], build)
    try:
        r.set_instances(M)
        assert_pairs(run(r, q), want, what)
    finally:
        r.close()
    return want


# 1. the soup under twelve transforms, near the origin and near 4 096
_SOUPS = {}


def soup_case(offset):
    """(triangles, transforms, sweeps, live, expected (records, instances)): a 64-triangle soup under regular_transforms(12), 384 aimed
    sweeps at each of RADII; made once and left unchanged"""
    if offset not in _SOUPS:
        rng = np.random.default_rng(41)
        tris = soup(rng, 64, edge=0.2)
        M = regular_transforms(12) if not offset else near_translations(regular_transforms(12), offset)
        live = live_of(M)
        q = np.concatenate([aimed_sweeps(rng, M, tris, 384, radius) for radius in RADII])
        _SOUPS[offset] = tris, M, q, live, expected(q, M, tris, pair_valid(12, 64, live))
    return _SOUPS[offset]


@pytest.mark.parametrize("offset", (0.0, 4096.0), ids=("near the origin", "near 4 096"))
def test_soup(native_lib, offset):
    tris, M, q, live, want = soup_case(offset)
    hit = want[1] >= 0
    print("soup at %g: %d hits of %d, %d instances win, %d start overlaps" % (offset, hit.sum(), len(q), len(np.unique(want[1][hit])), (want[0][hit, 3] == 0).sum()))
    assert 0.2 * len(q) < hit.sum() < 0.9 * len(q) and len(np.unique(want[1][hit])) >= 8
    r = context([tris])
    try:
        assert r.set_instances(M).inert == (~live).sum()
        assert_pairs(run(r, q), want, "soup at %g" % offset)
    finally:
        r.close()


# 2. scenes built against the prune
def test_sphere_under_a_scale_and_a_rotation(native_lib):
    """a sphere mesh under a non-uniform scale and a 45 degree rotation: from the image of its centre outward every subtree is almost
    equally far; from outside inward the sweep grazes many rotated boxes before the first contact"""
    rng = np.random.default_rng(42)
    tris = sphere(16, 16)
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    centre = np.float64([3, -2, 5])
    M = np.stack([affine(R @ np.diag([3.0, 1.0, 0.5]), centre)])
    d = rng.normal(size=(192, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = sweep_queries(centre + rng.normal(size=(192, 3)) * 1e-3, 0.05, d)
    start = centre + 6.0 * d + rng.normal(size=(192, 3)) * 0.3
    inward = sweep_queries(start, 0.1, -d * (0.5 + rng.random((192, 1))))
    inward[1::4, 7] = 4.0
    want = check(tris, M, np.concatenate([out, inward]), "sphere")
    assert (want[1][:192] == 0).all() and 100 < (want[1][192:] == 0).sum() < 192


def test_needles(native_lib):
    rng = np.random.default_rng(43)
    tris = needles(rng, 200)
    M = regular_transforms(6)
    q = np.concatenate([aimed_sweeps(rng, M, tris, 128, radius) for radius in RADII])
    want = check(tris, M, q, "needles")
    assert 50 < (want[1] >= 0).sum() < len(q)


def test_sixteen_instances_at_one_place(native_lib):
    """every world box holds every sweep's path: the winner is the lowest instance"""
    rng = np.random.default_rng(44)
    tris = soup(rng, 100, edge=0.2)
    M = np.tile(affine(rotation(rng), (5, 6, 7)), (16, 1, 1))
    q = np.concatenate([aimed_sweeps(rng, M, tris, 96, radius) for radius in RADII])
    want = check(tris, M, q, "16 instances at one place")
    assert (want[1] >= 0).sum() > 60 and (want[1] <= 0).all()


def test_known_answers(native_lib):
    cases = known_cases()
    for M in {c[1].tobytes(): c[1] for c in cases}.values():
        mine = [c for c in cases if c[1].tobytes() == M.tobytes()]
        q, want = np.stack([c[2] for c in mine]), np.stack([c[3] for c in mine])
        r = context([TRI])
        try:
            r.set_instances(M[None])
            rec, inst = run(r, q)
            assert_records(rec, want, "known answers, " + mine[0][0])
            assert (inst == 0).all()
        finally:
            r.close()


# 3. ties
def test_ties_go_to_the_lower_instance_then_the_lower_id(native_lib):
    n = 12
    _, quads = stacked_quads(n, 0.25)
    tris = np.concatenate([quads, quads])  # every triangle twice
    A = affine(ROT90, (8, 0, 0))
    top = (n - 1) * 0.25
    upside_down = affine(np.diag([1.0, 1.0, -1.0]) @ np.float64(ROT90), (8, 0, top))  # its quad k lies where A's quad n - 1 - k does
    M = np.stack([affine(np.eye(3), (100, 0, 0)), A, A, upside_down])
    xy = [(0.5, 0.5), (0.25, 0.25), (0.75, 0.75), (0.5, 0.25), (0.25, 0.5), (0, 0), (1, 1), (1.125, 0.5), (0.5, -0.125)]
    o = np.float64([(x, y, z) for x, y in xy for z in (top + 2.0, -2.0)])
    d = [(0, 0, -1 if z > 0 else 1) for _, _, z in o]
    o = o @ np.float64(ROT90).T + np.float64([8, 0, 0])
    q = np.concatenate([sweep_queries(o, 0.25, d), sweep_queries(o, 0.0, d)])
    rec, inst, table = sweep_instances(q, M, tris)
    hit = inst >= 0
    tied = (table == rec[:, 3][:, None, None])[hit]
    assert hit.sum() > 0.8 * len(q) and (tied.sum((1, 2)) >= 6).all(), "two coinciding instances, a third that ties with another triangle, doubled triangles"
    assert (inst[hit] == 1).all() and (bits(rec)[hit, 6] < len(quads)).all() and tied[:, 3].any(1).all()
    r = context([tris])
    try:
        r.set_instances(M)
        assert_pairs(run(r, q), (rec, inst), "ties")
    finally:
        r.close()


# 4. tmax
def test_tmax_at_the_answer_and_one_ulp_below(native_lib):
    tris, M, q, live, want = soup_case(0.0)
    moving = (want[1] >= 0) & (want[0][:, 3] > 0)
    q = q[moving][:192].copy()
    at = want[0][moving][:192, 3]
    valid = pair_valid(12, 64, live)
    r = context([tris])
    try:
        r.set_instances(M)
        hits = {}
        for name, tmax in (("at", at), ("below", np.nextafter(at, f32(0)))):
            q[:, 7] = tmax
            w = expected(q, M, tris, valid)
            hits[name] = w[1] >= 0
            assert (w[0][~hits[name], 3] == q[~hits[name], 7]).all(), "the miss record carries tmax"
            assert_pairs(run(r, q), w, "tmax " + name)
        assert hits["at"].all() and hits["below"].sum() < 0.5 * len(q), "t <= tmax is inclusive, and the first contact is the first"
    finally:
        r.close()


# 5. degenerate sweeps, sizes
@pytest.fixture(scope="module")
def small_case():
    """the soup's first 512 sweeps with degenerate ones between the good ones; the brute force, once"""
    tris, M, q, live, _ = soup_case(0.0)
    q = np.concatenate([q[:256], q[768:1024]]).copy()
    bad = degenerate_sweeps()
    q[3::51][:len(bad)] = bad
    want = expected(q, M, tris, pair_valid(12, 64, live))
    miss = np.zeros(8, np.uint32)
    miss[6] = MISS
    assert (bits(want[0])[3::51][:len(bad)] == miss).all() and (want[1][3::51][:len(bad)] == -1).all() and 100 < (want[1] >= 0).sum() < 500
    return tris, M, q, want


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_sizes_with_degenerate_sweeps_and_canaries(native_lib, small_case, n):
    import torch
    tris, M, q, want = small_case
    reps = -(-n // len(q))
    qn, wn, wi = np.tile(q, (reps, 1))[:n], np.tile(want[0], (reps, 1))[:n], np.tile(want[1], reps)[:n]
    dev = torch.device("cuda", 0)
    out = torch.full((n + 8, 8), CANARY, dtype=torch.int32, device=dev)
    ins = torch.full((n + 8,), CANARY, dtype=torch.int32, device=dev)
    sw = torch.as_tensor(qn, device=dev).contiguous()
    L = capi.lib()
    r = context([tris])
    try:
        r.set_instances(M)
        torch.cuda.synchronize()
        assert L.cap_sweep_instances(r.ctx, sw.data_ptr(), n, out.data_ptr(), ins.data_ptr(), None) == 0
        r.sync()
        got, gi = out.view(torch.float32).cpu().numpy(), ins.cpu().numpy()
        assert_pairs((got[:n], gi[:n]), (wn, wi), "n = %d" % n)
        assert (bits(got[n:]) == CANARY).all() and (gi[n:].view(np.uint32) == CANARY).all(), "nothing behind the last record or instance"
        # device_instances = NULL
        out2 = torch.full((n + 8, 8), CANARY, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert L.cap_sweep_instances(r.ctx, sw.data_ptr(), n, out2.data_ptr(), None, None) == 0
        r.sync()
        assert bool((out2 == out).all())
    finally:
        r.close()


@pytest.mark.parametrize("count", (1, 2, 3, 5))
def test_few_instances_of_a_one_triangle_scene(native_lib, count):
    """1, 2, 3 and 5 instances exercise the top level's padding; the one-triangle scene has a leaf for a root"""
    rng = np.random.default_rng(45)
    M = regular_transforms(6)[1:1 + count]
    tris = soup(rng, 1, edge=0.5)
    q = np.concatenate([aimed_sweeps(rng, M, tris, 96, radius, jitter=0.3) for radius in (0.03, 0.3)])
    want = check(tris, M, q, "%d instances of one triangle" % count)
    assert 20 < (want[1] >= 0).sum() < len(q) and len(np.unique(want[1][want[1] >= 0])) == count


# 6. builders
@pytest.mark.parametrize("build", (B.BVH_BUILD_LBVH, B.BVH_BUILD_SAH, B.BVH_BUILD_SAH_DEVICE), ids=("lbvh", "sah", "sah_device"))
def test_every_builder_equals_the_brute_force(native_lib, build):
    tris, M, q, live, want = soup_case(0.0)
    r = context([tris], build)
    try:
        r.set_instances(M)
        assert_pairs(run(r, q[::3]), (want[0][::3], want[1][::3]), "builder %d" % build)
    finally:
        r.close()


# 7. extreme transforms, from host and from device descriptors
def test_extreme_transforms_host_and_device(native_lib):
    import torch
    rng = np.random.default_rng(46)
    tris = soup(rng, 100, edge=0.2)
    M, must_be_inert = extreme_transforms()
    M, must_be_inert = np.concatenate([M, regular_transforms(3)]), np.concatenate([must_be_inert, np.zeros(3, bool)])
    live = live_of(M)
    assert not live[must_be_inert].any() and live.sum() >= 4 and (~live).sum() >= 1
    q = np.concatenate([aimed_sweeps(rng, M[live], tris, 96, radius) for radius in RADII])
    want = expected(q, M, tris, pair_valid(len(M), len(tris), live))
    hit = want[1] >= 0
    assert hit.sum() > 60 and live[want[1][hit]].all() and len(np.unique(want[1][hit])) >= 3
    r = context([tris])
    try:
        info = r.set_instances(M)
        assert info.inert == (~live).sum(), "the debug entry decides as the device does"
        assert_pairs(run(r, q), want, "host descriptors")
        r.set_instances(torch.as_tensor(M, device=torch.device("cuda", 0)))
        assert_pairs(run(r, q), want, "device descriptors")
    finally:
        r.close()


# 8. objects
@pytest.mark.parametrize("count", (2, 3))
def test_objects(native_lib, count):
    rng = np.random.default_rng(47)
    parts = [arrays(soup(rng, 60, edge=0.2)), arrays(soup(rng, 40, edge=0.2, offset=0.5), soup(rng, 20, edge=0.3)), single_triangle()][:count]
    scene, ranges = concat(parts)
    tris = scene_triangles(scene)
    tr = triangle_ranges(scene[4], ranges)
    obj_of_tri = np.concatenate([np.full(n, k) for k, (f, n) in enumerate(tr)])
    M = regular_transforms(12)
    objects = np.arange(12) % count
    q = np.concatenate([aimed_sweeps(rng, M, tris, 144, radius) for radius in (0.03, 0.1)])
    want = expected(q, M, tris, pair_valid(12, len(tris), None, None, None, None, objects, obj_of_tri))
    hit = want[1] >= 0
    assert hit.sum() > 60 and (obj_of_tri[bits(want[0])[hit, 6]] == objects[want[1][hit]]).all()
    assert len(np.unique(objects[want[1][hit]])) == count, "every object answers somewhere"
    whole = expected(q, M, tris)
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


# 9. masks
def test_masks_and_option_errors(native_lib):
    import torch
    rng = np.random.default_rng(48)
    a, b = soup(rng, 50, edge=0.2), soup(rng, 50, edge=0.2)
    tris = np.concatenate([a, b])
    M = regular_transforms(8)
    imasks = np.uint32([0x01, 0x02, 0x04, 0xFF, 0x03, 0x00, 0x01, 0x02])
    q = np.concatenate([aimed_sweeps(rng, M, tris, 128, radius) for radius in (0.03, 0.1)])
    mesh_of_tri = (np.arange(100) >= 50).astype(np.int64)

    def ref(inst_masks=None, mesh_masks=None, mask=None):
        tm = None if mesh_masks is None else np.uint32(mesh_masks)[mesh_of_tri]
        return expected(q, M, tris, pair_valid(8, 100, None, inst_masks, tm, mask))

    dev = torch.device("cuda", 0)
    r = context([a, b])
    try:
        r.set_instances(M, masks=imasks)
        want = ref(imasks)
        assert (want[1] != 5).all() and (want[1] >= 0).sum() > 40 and not np.array_equal(bits(want[0]), bits(ref()[0]))
        assert_pairs(run(r, q), want, "instance masks")
        assert_pairs(run(r, q, mask=0x01), ref(imasks, None, 0x01), "instance masks and the call's mask")
        assert_pairs(run(r, q, mask=0x08), ref(imasks, None, 0x08), "a call mask only 0xFF passes")
        r.set_instance_masks([0x05, 0x02])
        assert_pairs(run(r, q), ref(imasks, [0x05, 0x02]), "instance and mesh masks")
        assert_pairs(run(r, q, mask=0x06), ref(imasks, [0x05, 0x02], 0x06), "instance, mesh and call masks")
        r.set_instance_masks([0x00, 0xFF])
        only_b = ref(imasks, [0x00, 0xFF])
        assert (bits(only_b[0])[only_b[1] >= 0, 6] >= 50).all()
        assert_pairs(run(r, q), only_b, "a mesh with mask 0 is invisible")
        r.set_instance_masks([0x00, 0x00])
        none = run(r, q)
        assert (none[1] == -1).all() and (bits(none[0])[:, 6] == MISS).all() and np.array_equal(none[0][:, 3], q[:, 7])
        r.set_instance_masks(None)
        r.set_instances(M, masks=np.zeros(8, np.uint32))
        none = run(r, q)
        assert (none[1] == -1).all() and (bits(none[0])[:, 6] == MISS).all(), "mask 0 on every instance: all misses"
        r.set_instances(M, masks=imasks)

        # options the call refuses: nothing is written
        L = capi.lib()
        sw = torch.as_tensor(q, device=dev).contiguous()
        out = torch.full((len(q), 8), CANARY, dtype=torch.int32, device=dev)
        ins = torch.full((len(q),), CANARY, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        call = lambda *o: L.cap_sweep_instances(r.ctx, sw.data_ptr(), len(q), out.data_ptr(), ins.data_ptr(),
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
            r.sweep_instances(q, mask=0x100)
    finally:
        r.close()


# 10. the three identities, on the device
def test_identities_on_the_device(native_lib):
    rng = np.random.default_rng(49)
    scene, tris = grid_scene(30)
    T = len(tris)
    tr = f32([[0, 0, 0], [16, 0, 0], [0, 0, 0], [-32, 16, 48], [64, -64, 16], [16, 0, 0], [-64, 64, -64]])  # coinciding copies
    o = rng.integers(-100 * 16, 100 * 16 + 1, (384, 3)) / 16.0
    aim = tr[rng.integers(0, len(tr), 384)] + rng.integers(-8 * 16, 8 * 16 + 1, (384, 3)) / 16.0
    q = sweep_queries(o, rng.integers(1, 64, 384) / 16.0, (aim - o) / 16.0, rng.integers(8, 64, 384) / 2.0)
    r = capi.Renderer(0)
    flat = capi.Renderer(0)
    try:
        r.upload_scene(*scene)
        r.build_bvh()
        # 1. one identity instance is the scene form (the grid scene has no -0 coordinate)
        assert not (bits(tris) == 0x80000000).any()
        r.set_instances(identity())
        rec, inst = run(r, q)
        plain = r.sweep_spheres(q)
        assert_records(rec, plain, "identity instance against cap_sweep_spheres")
        assert ((inst == 0) == (bits(plain)[:, 6] != MISS)).all() and ((inst == -1) | (inst == 0)).all() and 0 < (inst == 0).sum() < len(q)
        # 2. translations on the grid are the flattened scene
        r.set_instances(translations(tr))
        rec, inst = run(r, q)
        flat.upload_scene(*flatten(scene, tr))
        flat.build_bvh()
        assert_records(flat_record(rec, inst, T), flat.sweep_spheres(q), "translations against the flattened scene")
        assert len(np.unique(inst)) >= 5 and (inst == 2).sum() == 0 and (inst == 5).sum() == 0 and (inst == -1).sum() > 0
        assert_pairs((rec, inst), expected(q, translations(tr), tris), "translations against the brute force")
        # 3. everything scaled by a power of two
        M = regular_transforms(8)
        qs = aimed_sweeps(rng, M, tris, 256, 0.03)
        r.set_instances(M)
        rec, inst = run(r, qs)
        assert 0 < (inst >= 0).sum() < len(qs)
        for j in (3, -2):
            s = f32(2.0 ** j)
            scaled = qs.copy()
            scaled[:, 0:7] *= s
            r.set_instances(M * s)
            rec_s, inst_s = run(r, scaled)
            assert np.array_equal(inst_s, inst) and np.array_equal(bits(rec_s)[:, 3:8], bits(rec)[:, 3:8])
            assert np.array_equal(bits(rec_s[:, 0:3]), bits(rec[:, 0:3] * s))
    finally:
        r.close()
        flat.close()


# 11. state and arguments
def test_state_refit_rebuild_and_replaced_tables(native_lib):
    rng = np.random.default_rng(50)
    a, b = soup(rng, 60, edge=0.2), soup(rng, 40, edge=0.2)
    tris = np.concatenate([a, b])
    M, M2 = regular_transforms(8), regular_transforms(8, seed=77)
    q = np.concatenate([aimed_sweeps(rng, M, tris, 96, radius) for radius in (0.03, 0.1)])
    P = arrays(a, b)[0]
    moved = (P + f32([0.05, -0.02, 0.03]) + (rng.random(P.shape) - 0.5).astype(f32) * f32(0.05)).astype(f32)
    want, want_moved, want2 = expected(q, M, tris), expected(q, M, moved.reshape(-1, 3, 3)), expected(q, M2, tris)
    assert not np.array_equal(bits(want[0]), bits(want_moved[0])) and not np.array_equal(bits(want[0]), bits(want2[0]))
    objects, obj_of_tri = np.arange(8) % 2, (np.arange(100) >= 60).astype(np.int64)
    want_obj = expected(q, M, moved.reshape(-1, 3, 3), pair_valid(8, 100, None, None, None, None, objects, obj_of_tri))
    r = context([a, b])
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
        r.set_objects([(0, 1), (1, 1)])
        r.set_instances(M, objects=objects)
        assert_pairs(run(r, q), want_obj, "a replaced object table")
        r.set_instances(None)
        with pytest.raises(capi.CapError, match="status 3"):
            run(r, q)
    finally:
        r.close()


def test_argument_contract(native_lib):
    import torch
    tris, M, q, live, want = soup_case(0.0)
    dev = torch.device("cuda", 0)
    L = capi.lib()
    n = 128
    sw = torch.as_tensor(q[:n], device=dev).contiguous()
    out = torch.full((n + 8, 8), CANARY, dtype=torch.int32, device=dev)
    ins = torch.full((n + 8,), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    P, O, I = sw.data_ptr(), out.data_ptr(), ins.data_ptr()
    r = capi.Renderer(0)
    try:
        call = lambda p=P, m=n, o=O, i=I: L.cap_sweep_instances(r.ctx, p, m, o, i, None)
        assert call() == ERR_STATE and b"cap_bvh_build" in L.cap_last_error()  # nothing uploaded
        r.upload_scene(*arrays(tris))
        r.build_bvh()
        assert call() == ERR_STATE and b"cap_instances_set" in L.cap_last_error() and call(P, 0) == ERR_STATE  # the state comes before n == 0
        r.set_instances(M)
        assert L.cap_sweep_instances(None, P, n, O, I, None) == ERR_INVALID_ARG
        assert call(None) == ERR_INVALID_ARG and call(P, n, None) == ERR_INVALID_ARG and b"NULL" in L.cap_last_error()
        assert call(P + 4) == ERR_INVALID_ARG and b"sweeps is not 16-byte aligned" in L.cap_last_error()
        assert call(P, n, O + 8) == ERR_INVALID_ARG and b"hits is not 16-byte aligned" in L.cap_last_error()
        assert call(P, n, O, I + 2) == ERR_INVALID_ARG and b"instances is not 4-byte aligned" in L.cap_last_error()
        assert call(P, n, P) == ERR_INVALID_ARG and call(P, n, P + 32 * (n - 1) + 16) == ERR_INVALID_ARG and b"overlap" in L.cap_last_error()
        assert call(O + 32 * (n - 1) + 16, n, O) == ERR_INVALID_ARG
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
            r.sweep_instances(torch.zeros((4, 4), device=dev))
        with pytest.raises(capi.CapError):
            r.sweep_instances(sw, out=torch.zeros((n, 4), device=dev))
    finally:
        r.close()


# 12. the contact is the closest-point function's
def test_each_hit_is_what_closest_instances_says_at_the_contact_centre(native_lib):
    """closest_instances at c = o + t d (at o itself for t = 0), with the winning pair alone unmasked -- the winner's instance by its
    mask bit, the winner's triangle by its mesh -- returns the hit's point, u, v, triangle, feature and instance; its dist2 is within
    the acceptance bound"""
    tris, M, q, live, _ = soup_case(0.0)
    tris, M, q = tris[:24], M[:8], q[::4]
    want = expected(q, M, tris)
    r = context([t[None] for t in tris])  # one mesh per triangle
    try:
        r.set_instances(M, masks=np.uint32(1) << np.arange(8).astype(np.uint32))  # instance i answers to bit i alone
        rec, inst = run(r, q)
        assert_pairs((rec, inst), want, "one mesh per triangle, one mask bit per instance")
        ids = bits(rec)[:, 6]
        t = rec[:, 3:4]
        c = np.where(t == 0, q[:, 0:3], q[:, 0:3] + t * q[:, 4:7]).astype(f32)
        seen = 0
        for i, g in sorted({(int(i), int(g)) for i, g in zip(inst, ids) if i >= 0}):
            rows = np.nonzero((inst == i) & (ids == g))[0]
            masks = np.zeros(len(tris), np.uint8)
            masks[g] = 0xFF
            r.set_instance_masks(masks)
            near, near_inst = r.closest_instances(queries(c[rows]), mask=1 << i)
            assert np.array_equal(bits(near)[:, [0, 1, 2, 4, 5, 6, 7]], bits(rec)[rows][:, [0, 1, 2, 4, 5, 6, 7]]) and (near_inst == i).all(), (i, g)
            r2 = q[rows, 3] * q[rows, 3]
            assert (near[:, 3] <= r2 * (f32(1) + f32(8) * f32(2.0 ** -24))).all()
            seen += len(rows)
        assert seen > 40
    finally:
        r.close()


def test_a_render_is_unchanged_by_a_query_between_its_batches(native_lib, bluenoise, cornell_path):
    geo = capi.Geometry(cornell_path)
    cam = capi.cornell_camera(64, 64)
    rng = np.random.default_rng(5)
    M = np.stack([identity()[0], affine(rotation(rng) * 0.5, (300, 100, -200)), affine(np.diag([1.0, 2.0, 0.5]), (-50, 20, 10))])
    d = rng.normal(size=(300, 3))
    q = sweep_queries(rng.random((300, 3)) * 700.0 - 100.0, 5.0 + 20.0 * rng.random(300), d / np.linalg.norm(d, axis=1, keepdims=True))
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
                got = r.sweep_instances(q)
                after = (bits(r.readback(capi.BUF_ACCUM_SUM)), r.stats().as_dict())
                assert np.array_equal(before[0], after[0])
                assert {k: v for k, v in before[1].items() if not k.startswith("ms_")} == {k: v for k, v in after[1].items() if not k.startswith("ms_")}
                P = geo.positions.reshape(-1, 3)
                tris = np.concatenate([P[geo.indices[int(m[3]):int(m[3]) + int(m[2])].astype(np.int64) + int(m[1])].reshape(-1, 3, 3) for m in geo.meshes])
                assert_pairs(got, expected(q, M, tris), "the Cornell box under three instances")
            r.render(2, 2, 2, capi.RENDER_AOV)
            s = r.stats()
            result.append((bits(r.readback(capi.BUF_ACCUM_SUM)), (s.rays_primary, s.rays_extension, s.rays_shadow, s.shaded_vertices, s.frames)))
        finally:
            r.close()
    assert np.array_equal(result[0][0], result[1][0]) and result[0][1] == result[1][1]
