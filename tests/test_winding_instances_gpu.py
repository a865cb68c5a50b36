"""Winding numbers over instances on the GPU (cap_winding_instances): the derived tables against their float64 definition
(winding_instances_support), the query against the host restatement of its two-level walk on the read-backs -- visit counts bit for bit
against walk32, values within a tolerance made of the float32 restatement's own error against walk, and against the float64 brute force
over the flattened scene at beta = inf --, the identity with cap_winding_numbers, the life cycle of the derived tables, the argument
contract, and Renderer.signed_distance_instances(sign="winding")."""
import functools

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import arrays, bits, closest, context, queries
from signed_distance_support import box, mesh, winding_number
from winding_instances_support import (EMPTY, IDENTITY, State, affine, brute_force, contributes, grid_transforms, instance_records, level_offsets, off_surface,
                                       points_about, rotation, top_moments, walk, walk32, world_triangles)
from winding_support import child_boxes, children, moments, octant_triangle, open_cube, overflow_scene, punctured, root_code, triangle_sums, unit_sphere

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 3
CANARY = 0x7FC0BEEF  # a NaN pattern no winding number and no count holds


# ---- the cases ----
def mixed_transforms():
    rng = np.random.default_rng(21)
    shear = np.array([[1.0, 0.4, 0.0], [0.0, 1.25, -0.3], [0.0, 0.0, 0.75]])
    return np.stack([IDENTITY, affine(rotation(rng) @ np.diag([0.5, 1.0, 1.5]), (3, 0, 0)), affine(shear, (0, 3, 0)),
                     affine(rotation(rng) @ np.diag([1.0, 1.0, -1.0]), (0, 0, 3)), affine(2.0 * np.eye(3), (4096, 0, 0))])


def three_parts():
    parts = [mesh("tetrahedron"), (mesh("torus") + np.float32([8, 0, 0])).astype(np.float32), (octant_triangle() + np.float32([0, 8, 0])).astype(np.float32)]
    ranges = [(0, len(parts[0])), (len(parts[0]), len(parts[1])), (len(parts[0]) + len(parts[1]), 1)]
    return parts, ranges


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (triangle sets, transforms, masks or None, object of every instance or None)"""
    mixed = mixed_transforms()
    singular = affine(np.diag([1.0, 1.0, 0.0]), (6, 6, 6))  # not invertible: inert
    return {
        "identity": ([mesh("torus")], IDENTITY[None], None, None),
        "two": ([open_cube()], mixed[:2], None, None),
        "three": ([mesh("tetrahedron")], mixed[:3], None, None),
        "five": ([box((1.0, 2.0, 3.0))], mixed, None, None),
        "one triangle": ([octant_triangle()], mixed[:3], None, None),
        "grid": ([open_cube()], grid_transforms(4), None, None),
        "inert and masked": ([open_cube()], np.concatenate([mixed[:3], singular[None], mixed[3:4]]), [0xFF, 0x00, 0x01, 0xFF, 0x80], None),
        "objects": (three_parts()[0], np.concatenate([mixed[:4], mixed[1:3]]), None, [0, 1, 2, 1, 2, 0]),
    }


def scene_of(name, build=None):
    """(renderer with the tree, the table, the objects and the instances of the case; tris, M, masks, ranges, objects)"""
    sets, M, masks, objects = cases()[name]
    r = context(sets, build)
    r.build_winding()
    ranges = None
    if objects is not None:
        r.set_objects([(k, 1) for k in range(len(sets))])
        first = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
        ranges = [(int(first[k]), len(sets[k])) for k in range(len(sets))]
    r.set_instances(M, masks, objects=objects)
    return r, np.concatenate(sets).astype(np.float32), M, (np.full(len(M), 0xFF) if masks is None else np.asarray(masks)), ranges, objects


def device_state(r, tris, M, ranges, objects):
    """the State of the walk from the read-backs, and the info"""
    top, inst, forest = r.winding_instances_tables()
    info = r.winding_instances_info()
    W, _ = r.instances_readback()
    if ranges is None:
        (nodes, order), table = r.bvh_readback(), r.winding_table()
        roots = [root_code(len(tris))] * len(M)
    else:
        (nodes, order), table = r.objects_readback(), forest
        nb = np.concatenate([[0], np.cumsum([c - 1 for _, c in ranges])])
        rb = np.concatenate([[0], np.cumsum([c for _, c in ranges])])
        roots = [int(nb[o]) if ranges[o][1] >= 2 else ~int(rb[o]) for o in objects]
    return State(top, list(info.level_entries)[:info.levels], inst, W, roots, table, order, tris, M), info, nodes


def assert_tables(r, tris, M, masks, ranges, objects, what):
    """the three derived tables against the float64 definition on the device's own trees and boxes; returns (State, on)"""
    st, info, nodes = device_state(r, tris, M, ranges, objects)
    W, boxes = r.instances_readback()
    on = contributes(M, masks, (W != 0).any((1, 2)))
    I = len(M)
    assert info.built == 1 and info.instances == I and info.contributing == on.sum(), what
    off, levels = level_offsets(st.level_entries)
    assert levels == info.levels and off[-1] == info.entries == len(st.top), what
    # per instance
    ref = instance_records(M, on)
    assert np.array_equal(bits(st.inst[:, 0:9]), bits(ref[:, 0:9].astype(np.float32))), "%s: L is the descriptor's, bit for bit" % what
    assert np.array_equal(st.inst[:, 11], ref[:, 11].astype(np.float32)), "%s: s" % what
    fin = np.isfinite(ref[:, 9])
    assert (np.abs(st.inst[fin, 9] - ref[fin, 9]) <= 2.0 ** -23 * ref[fin, 9]).all(), "%s: |det L|" % what
    sg = st.inst[:, 10].astype(np.float64)
    assert (sg >= ref[:, 10]).all() and (sg <= ref[:, 10] * (1 + 2.0 ** -22)).all(), "%s: sigma is rounded up, and not by much" % what
    assert (sg[on] >= np.linalg.norm(ref[on, 0:9].reshape(-1, 3, 3), 2, axis=(1, 2)) * (1 - 1e-15)).all(), "%s: sigma bounds the 2-norm" % what
    # the objects' table (the scene's own without an object table: test_winding_gpu checks that one)
    if ranges is not None and len(st.table32):
        t64, want = moments(nodes, st.order, tris)
        assert np.array_equal(st.table32.view(np.int32)[:, :, 7], children(nodes)), "%s: word 7 of the forest's table is the forest's child code" % what
        cb = child_boxes(nodes).astype(np.float64)
        mag = np.abs(cb).max((2, 3))
        p, rad, N = st.table32[:, :, 0:3].astype(np.float64), st.table32[:, :, 3].astype(np.float64), st.table32[:, :, 4:7].astype(np.float64)
        assert (np.abs(p - t64[:, :, 0:3]).max(2) <= 2.0 ** -22 * mag).all(), "%s: forest p~" % what
        assert (np.abs(N - t64[:, :, 4:7]).max(2) <= 2.0 ** -22 * want["areas"]).all(), "%s: forest N" % what
        far = np.sqrt((np.maximum(np.abs(cb[:, :, 0] - p), np.abs(cb[:, :, 1] - p)) ** 2).sum(2))
        assert (rad >= far).all() and (rad <= far * (1 + 2.0 ** -21)).all(), "%s: forest r" % what
    # the top level
    word7 = st.top.view(np.uint32)[:, 7]
    n0 = I + (I & 1)
    assert sorted(word7[:I].tolist()) == list(range(I)) and (word7[I:] == EMPTY).all(), "%s: word 7, bit for bit: level 0 holds every instance once" % what
    if I <= 2:
        assert word7[:I].tolist() == list(range(I)), what
    rng = [(0, len(tris))] * I if ranges is None else [ranges[o] for o in objects]
    obj_sums = np.stack([triangle_sums(tris[f:f + c])[0].sum(0) for f, c in rng])
    order0 = word7[:n0].astype(np.int64).tolist()
    t64, ex = top_moments(M, on, order0, obj_sums, boxes.astype(np.float64), st.level_entries)
    full = ex["full"]
    assert np.array_equal(st.top[:, 3] >= 0, full), "%s: exactly the entries without a contributing instance are empty" % what
    assert (st.top[~full, 0:7] == np.float32([0, 0, 0, -1, 0, 0, 0])).all(), what
    p, rad, N = st.top[full, 0:3].astype(np.float64), st.top[full, 3].astype(np.float64), st.top[full, 4:7].astype(np.float64)
    lo, hi = ex["lo"][full], ex["hi"][full]
    mag = np.maximum(np.abs(lo), np.abs(hi)).max(1)
    assert (np.abs(p - t64[full, 0:3]).max(1) <= 2.0 ** -22 * mag).all(), "%s: p~_w" % what
    assert (np.abs(N - t64[full, 4:7]).max(1) <= 2.0 ** -22 * ex["nbound"][full]).all(), "%s: N_w" % what
    far = np.sqrt((np.maximum(np.abs(lo - p), np.abs(hi - p)) ** 2).sum(1))  # from the STORED p~_w
    assert (rad >= far).all() and (rad <= far * (1 + 2.0 ** -21)).all(), "%s: r covers the entry's stored box and not much more" % what
    root = int(off[levels - 1])
    assert info.total_weight == pytest.approx(ex["weight"][root], rel=1e-12), what
    assert np.array_equal(np.float32(list(info.root_n)), st.top[root, 4:7]) and np.array_equal(np.float32(list(info.root_p)), st.top[root, 0:3]), what
    return st, on


def raw_call(r, q, beta, with_visits=True, pad=8):
    """cap_winding_instances on device buffers with canaries behind both outputs: (w float32, visits (N, 4) or None), canaries checked"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(q)
    pts = torch.as_tensor(np.array(q, np.float32), device=dev).contiguous()
    out = torch.full((n + pad,), CANARY, dtype=torch.int32, device=dev)
    vis = torch.full((n + pad, 4), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = capi.lib().cap_winding_instances(r.ctx, pts.data_ptr(), n, beta, out.data_ptr(), vis.data_ptr() if with_visits else None)
    assert rc == 0, capi.lib().cap_last_error()
    r.sync()
    o, v = out.cpu().numpy(), vis.cpu().numpy()
    assert (o[n:] == CANARY).all() and (v[n:] == CANARY).all(), "nothing behind the last value or count"
    if not with_visits:
        assert (v == CANARY).all()
    return o[:n].view(np.float32), (v[:n] if with_visits else None)


def assert_query(r, st, on, pts, keep, ranges, objects, betas, what, repeat=True):
    """visits bit for bit against walk32; values within max(8 x the host-measured |walk32 - walk| of the case, visits 2^-24) of walk; at
    beta = inf also of the brute force"""
    for beta in betas:
        want, want_visits = walk(st, pts, beta)
        w32, v32 = walk32(st, pts, beta)
        assert np.array_equal(v32, want_visits)
        got, visits = raw_call(r, pts, beta)
        assert np.array_equal(visits.astype(np.int64), v32), "%s beta %s: visits" % (what, beta)
        measured = np.abs(w32 - want)[keep].max()
        tol = np.maximum(8.0 * measured, want_visits.sum(1) * 2.0 ** -24)
        err = np.abs(got.astype(np.float64) - want)
        print("%s beta %s: max |gpu - walk| %.3e, host |walk32 - walk| %.3e (bound %.3e), mean visits %s" % (
            what, beta, err[keep].max(), measured, tol.min(), want_visits.mean(0).round(1).tolist()))
        assert (err[keep] <= tol[keep]).all(), "%s beta %s: %d values off, worst %.3e" % (what, beta, (err[keep] > tol[keep]).sum(), err[keep].max())
        if np.isinf(beta):
            assert (visits[:, 0] == 0).all() and (visits[:, 2] == 0).all() and (visits[:, 1] == on.sum()).all()
            truth = brute_force(pts, st.M, on, st.tris, ranges, objects)
            assert (np.abs(got.astype(np.float64) - truth)[keep] <= tol[keep]).all(), "%s: the exact sum against the brute force" % what
        if repeat:
            again, _ = raw_call(r, pts, beta)
            assert np.array_equal(bits(again), bits(got)), "two runs give the same bits"
            plain, _ = raw_call(r, pts, beta, with_visits=False)
            assert np.array_equal(bits(plain), bits(got)), "the same values without the visits array"


def case_points(M, on, tris, ranges, objects, n=300, seed=5):
    """n points, an equal share about each of the first eight contributing instances (its own world bounds grown by 0.5, so that an
    instance 4096 away gets its points too), and the mask of the ones off the surface of the whole flattened scene"""
    rng = np.random.default_rng(seed)
    first = np.nonzero(on)[0][:8]
    q = []
    for i in first:
        one = np.zeros(len(M), bool)
        one[i] = True
        q.append(points_about(rng, M, one, tris, -(-n // len(first)), ranges=ranges, objects=objects))
    q = np.concatenate(q)[:n]
    return q, off_surface(q, M, on, tris, ranges, objects)


# ---- 1. tables and query ----
@pytest.mark.parametrize("name", tuple(cases()))
def test_tables_and_query(native_lib, name):
    r, tris, M, masks, ranges, objects = scene_of(name)
    try:
        assert r.winding_instances_info().built == 0, "nothing is derived before the first query"
        scene_table = r.winding_table()
        st, on = assert_tables(r, tris, M, masks, ranges, objects, name)
        q, keep = case_points(M, on, tris, ranges, objects)
        assert keep.mean() >= 0.9
        assert_query(r, st, on, q, keep, ranges, objects, (2.0, np.inf), name)
        if name == "grid":
            assert walk32(st, q, 2.0)[1][:, 0].mean() > 1.0 and r.winding_instances_info().levels == 7, "several levels, with far terms taken there"
        if name == "inert and masked":
            assert on.tolist() == [True, False, True, False, True]
        assert np.array_equal(bits(r.winding_table()), bits(scene_table)), "the scene table's bytes are unchanged"
    finally:
        r.close()


@pytest.mark.parametrize("build", (capi.Renderer.BVH_BUILD_LBVH, capi.Renderer.BVH_BUILD_PLOC, capi.Renderer.BVH_BUILD_SAH_DEVICE))
def test_objects_on_every_device_builder(native_lib, build):
    r, tris, M, masks, ranges, objects = scene_of("objects", build)
    try:
        st, on = assert_tables(r, tris, M, masks, ranges, objects, "builder %d" % build)
        q, keep = case_points(M, on, tris, ranges, objects, n=200)
        assert_query(r, st, on, q, keep, ranges, objects, (2.0,), "objects, builder %d" % build, repeat=False)
    finally:
        r.close()


def test_known_answers(native_lib):
    mirror = affine(np.diag([1.0, 1.0, -1.0]), (0, 0, 3))
    cases_ = (("a mirrored closed box", box((1.0, 2.0, 3.0)), mirror[None], (0.5, 1.0, 1.5), 1.0),
              ("two overlapping instances", box((1.0, 1.0, 1.0)), np.stack([IDENTITY, affine(np.eye(3), (0.5, 0, 0))]), (0.75, 0.5, 0.5), 2.0),
              ("an open cube stretched to height 3", open_cube(), affine(np.diag([1.0, 1.0, 3.0]), (0, 0, 0))[None], (0.5, 0.5, 1.5), None))
    for what, tris, M, at, want in cases_:
        r = context([tris])
        try:
            r.build_winding()
            r.set_instances(M)
            if want is None:
                want = winding_number(np.float64([at]), tris.astype(np.float64) * [1.0, 1.0, 3.0])[0]
                assert abs(want - 5.0 / 6.0) > 0.05
            for beta in (2.0, 4.0, np.inf):
                w, v = raw_call(r, queries(np.float32([at])), beta)
                # (the exact sum to float32 rounding; a finite beta to the 0.05 the header gives for beta = 2)
                assert abs(float(w[0]) - want) <= (1e-5 if np.isinf(beta) else 0.05), "%s beta %s: %r" % (what, beta, float(w[0]))
        finally:
            r.close()


# ---- 2. the identity ----
def test_one_identity_instance_is_the_scene_query(native_lib):
    tris = (mesh("torus") + np.float32([3, 3, 3])).astype(np.float32)
    assert not (np.signbit(tris) & (tris == 0)).any(), "no negative zero"
    rng = np.random.default_rng(12)
    q = points_about(rng, IDENTITY[None], np.ones(1, bool), tris, 400)
    q = np.concatenate([q, queries((rng.normal(size=(200, 3)) * 20 + 3).astype(np.float32))])
    r = context([tris])
    try:
        r.build_winding()
        r.set_instances(IDENTITY[None])
        for beta in (np.inf, 2.0):
            flat, fv = r.winding_numbers(q, beta=beta, visits=True)
            got, gv = raw_call(r, q, beta)
            same = np.ones(len(q), bool) if np.isinf(beta) else gv[:, 0] == 0
            assert same.sum() >= 300 and (np.isinf(beta) or (~same).sum() >= 50)
            assert np.array_equal(bits(got[same]), bits(flat[same])), "beta %s: cap_winding_numbers' bits" % beta
            assert np.array_equal(gv[same][:, 2:4], fv[same]) and (gv[same][:, 1] == 1).all()
    finally:
        r.close()


def test_far_term_overflow(native_lib):
    """cap_winding_instances leaves a NaN far term out, at the top level and below an instance (cap_winding_numbers adds it:
    test_winding_gpu.test_far_term_overflow has the scene and the reasons of the bounds).  One identity instance; expected: walk32 as it
    stands, visits bit for bit."""
    tris, pts = overflow_scene()
    r = context([tris])
    try:
        r.build_winding()
        r.set_instances(IDENTITY[None])
        got, visits = raw_call(r, pts, 2.0)
        st, _, _ = device_state(r, tris, IDENTITY[None], None, None)
        want, want_visits = walk32(st, pts, 2.0)
        print("far term overflow: gpu %r visits %r, walk32 %r visits %r" % (got.tolist(), visits.tolist(), want.tolist(), want_visits.tolist()))
        assert want_visits.tolist() == [[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 2]] and want[0] == 0.0 and want[1] == 0.0, "the case is what it was built to be"
        assert np.array_equal(visits.astype(np.int64), want_visits)
        assert not np.isnan(got).any() and bits(got[0:1])[0] == 0, "a NaN far term adds nothing: 0.0 with one far term"
        far_only = want_visits[:, 3] == 0
        assert np.array_equal(bits(got[far_only]), bits(want[far_only].astype(np.float32)))
        assert abs(float(got[2]) - want[2]) <= want_visits[2, 3] * 2.0 ** -22
    finally:
        r.close()


# ---- 3. the life cycle ----
def test_derived_tables_follow_every_change(native_lib):
    r, tris, M, masks, ranges, objects = scene_of("objects", capi.Renderer.BVH_BUILD_SAH_DEVICE)
    parts, _ = three_parts()
    try:
        L = capi.lib()
        info = r.winding_instances_info()
        assert info.built == 0 and info.instances == len(M) and info.contributing == 0, "a context that never queried has no derived tables"
        scene_table = r.winding_table()

        def check(tris, M, masks, ranges, objects, what):
            assert r.winding_instances_info().built == 0, "%s marks the tables dirty" % what
            st, on = assert_tables(r, tris, M, masks, ranges, objects, what)
            q, keep = case_points(M, on, tris, ranges, objects, n=150)
            assert_query(r, st, on, q, keep, ranges, objects, (2.0,), what, repeat=False)
            assert r.winding_instances_info().built == 1

        check(tris, M, masks, ranges, objects, "the first query")
        # cap_instances_set again: other transforms, one switched off
        M2, masks2 = M[::-1].copy(), np.array([0xFF, 0xFF, 0x00, 0xFF, 0xFF, 0xFF])
        r.set_instances(M2, masks2, objects=objects)
        check(tris, M2, masks2, ranges, objects, "cap_instances_set")
        # moved vertices and a refit
        shear = np.float32([[1.25, 0.0, 0.0], [0.2, 0.75, 0.0], [0.0, -0.3, 1.5]])
        P = arrays(*parts)[0]
        moved = (P @ shear).astype(np.float32)
        r.update_vertices(positions=moved)
        assert L.cap_winding_instances(r.ctx, None, 0, 2.0, None, None) == ERR_STATE, "stale trees"
        r.refit_bvh()
        moved_tris = moved.reshape(-1, 3, 3)
        check(moved_tris, M2, masks2, ranges, objects, "cap_bvh_refit")
        assert not np.array_equal(bits(r.winding_table()), bits(scene_table))
        # a rebuild by another builder
        r.set_bvh_build(capi.Renderer.BVH_BUILD_LBVH)
        r.build_bvh()
        check(moved_tris, M2, masks2, ranges, objects, "cap_bvh_build")
        scene_table = r.winding_table()
        # cap_winding_build again
        r.build_winding()
        check(moved_tris, M2, masks2, ranges, objects, "cap_winding_build")
        # cap_objects_set again: two objects, the torus and the tetrahedron swapped; it drops the instance table
        r.set_objects([(1, 1), (0, 1)])
        assert L.cap_winding_instances(r.ctx, None, 0, 2.0, None, None) == ERR_STATE and b"cap_instances_set" in L.cap_last_error()
        ranges2, objects2 = [ranges[1], ranges[0]], [0, 1, 0]
        r.set_instances(M2[:3], None, objects=objects2)
        check(moved_tris, M2[:3], np.full(3, 0xFF), ranges2, objects2, "cap_objects_set")
        # no object table: every instance shows the whole scene
        r.set_objects(None)
        r.set_instances(M2[:2])
        check(moved_tris, M2[:2], np.full(2, 0xFF), None, None, "cap_objects_set(none)")
        assert np.array_equal(bits(r.winding_table()), bits(scene_table)), "the scene table's bytes are unchanged by all of it"
        # the drop takes everything
        r.drop_winding()
        assert r.winding_instances_info().built == 0
        assert L.cap_winding_instances(r.ctx, None, 0, 2.0, None, None) == ERR_STATE and b"cap_winding_build" in L.cap_last_error()
        r.build_winding()
        check(moved_tris, M2[:2], np.full(2, 0xFF), None, None, "drop and build")
    finally:
        r.close()


# ---- 4. the contract ----
def test_argument_contract(native_lib):
    import torch
    tris = mesh("torus")
    dev = torch.device("cuda", 0)
    L = capi.lib()
    n = 128
    M = mixed_transforms()[:3]
    q = points_about(np.random.default_rng(3), M, np.ones(3, bool), tris, n)
    q[5, 0], q[9, 1], q[17, 2], q[33, 3] = np.nan, np.inf, -np.inf, np.nan  # (the radius is not read)
    pts = torch.as_tensor(q, device=dev).contiguous()
    out = torch.full((n + 8,), CANARY, dtype=torch.int32, device=dev)
    vis = torch.full((n + 8, 4), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    P, O, V = pts.data_ptr(), out.data_ptr(), vis.data_ptr()
    r = capi.Renderer(0)
    try:
        call = lambda p=P, m=n, beta=2.0, o=O, v=V: L.cap_winding_instances(r.ctx, p, m, beta, o, v)
        r.upload_scene(*arrays(tris))
        assert call() == ERR_STATE and b"cap_bvh_build" in L.cap_last_error()
        assert L.cap_winding_instances_readback(r.ctx, None, None, None) == ERR_STATE
        r.build_bvh()
        assert call() == ERR_STATE and call(P, 0) == ERR_STATE and b"cap_winding_build" in L.cap_last_error()  # the state comes before n == 0
        r.build_winding()
        assert call() == ERR_STATE and b"cap_instances_set" in L.cap_last_error()
        assert L.cap_winding_instances_readback(r.ctx, None, None, None) == ERR_STATE
        r.set_instances(M)
        assert L.cap_winding_instances(None, P, n, 2.0, O, V) == ERR_INVALID_ARG
        assert L.cap_winding_instances_info(None, None) == ERR_INVALID_ARG and L.cap_winding_instances_info(r.ctx, None) == ERR_INVALID_ARG
        assert L.cap_winding_instances_readback(None, None, None, None) == ERR_INVALID_ARG
        for beta in (0.5, float("nan"), -1.0, float("-inf"), 0.0, 0.99999994):
            assert call(beta=beta) == ERR_INVALID_ARG and b"beta" in L.cap_last_error(), beta
        assert call(None) == ERR_INVALID_ARG and call(P, n, 2.0, None) == ERR_INVALID_ARG and b"NULL" in L.cap_last_error()
        assert call(P + 4) == ERR_INVALID_ARG and b"points is not 16-byte aligned" in L.cap_last_error()
        assert call(P, n, 2.0, O + 2) == ERR_INVALID_ARG and b"winding is not 4-byte aligned" in L.cap_last_error()
        assert call(P, n, 2.0, O, V + 2) == ERR_INVALID_ARG and b"visits is not 4-byte aligned" in L.cap_last_error()
        assert call(P, n, 2.0, P) == ERR_INVALID_ARG and b"points and winding ranges overlap" in L.cap_last_error()
        assert call(P, n, 2.0, O, P + 16 * (n - 1)) == ERR_INVALID_ARG and b"points and visits ranges overlap" in L.cap_last_error()
        assert call(P, n, 2.0, O, O + 4 * (n - 1)) == ERR_INVALID_ARG and b"winding and visits ranges overlap" in L.cap_last_error()
        assert call(P, 1 << 60) == ERR_INVALID_ARG and b"address space" in L.cap_last_error()
        assert call(None, 0, 2.0, None, None) == 0  # nothing to do
        assert r.winding_instances_info().built == 0, "and nothing was derived for it"
        r.sync()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()) and bool((vis == CANARY).all()), "nothing is written on an error"
        assert call(beta=1.0) == 0 and call(beta=float("inf")) == 0 and call() == 0
        r.sync()
        got, gv = out.cpu().numpy(), vis.cpu().numpy()
        assert (got[n:] == CANARY).all() and (gv[n:] == CANARY).all()
        w = got[:n].view(np.float32)
        bad = np.array([5, 9, 17])
        assert np.isnan(w[bad]).all() and (gv[bad] == 0).all(), "a non-finite coordinate: a quiet NaN and zero visits"
        assert (got[bad] & 0x7FC00000 == 0x7FC00000).all()
        st, _, _ = device_state(r, tris, M, None, None)
        want, want_visits = walk32(st, q, 2.0)
        good = np.setdiff1d(np.arange(n), bad)
        assert np.array_equal(gv[:n].astype(np.int64), want_visits) and np.abs(w[good] - want[good]).max() <= 1e-4
        # no contributing instance: 0.0
        r.set_instances(M, [0, 0, 0])
        w0, v0 = raw_call(r, q[good], 2.0)
        assert (bits(w0) == 0).all() and not v0.any()
        with pytest.raises(capi.CapError):
            r.winding_instances(torch.zeros((4, 3), device=dev))
    finally:
        r.close()


def test_python_wrapper(native_lib):
    import torch
    r, tris, M, masks, ranges, objects = scene_of("five")
    try:
        q, _ = case_points(M, np.ones(len(M), bool), tris, None, None, n=100)
        w, v = r.winding_instances(q, visits=True)
        assert isinstance(w, np.ndarray) and w.dtype == np.float32 and v.shape == (len(q), 4)
        raw, raw_v = raw_call(r, q, 2.0)
        assert np.array_equal(bits(w), bits(raw)) and np.array_equal(v, raw_v), "beta defaults to 2"
        dev = torch.as_tensor(q, device="cuda:0").contiguous()
        out = torch.zeros((len(q),), dtype=torch.float32, device="cuda:0")
        assert r.winding_instances(dev, beta=float("inf"), out=out) is out
        assert set(r.winding_instances_info().as_dict()) == {"instances", "contributing", "levels", "entries", "forest_records", "built", "level_entries",
                                                             "total_weight", "root_n", "root_p"}
        with pytest.raises(capi.CapError, match="status 1"):
            r.winding_instances(q, beta=0.5)
    finally:
        r.close()


# ---- 5. signed_distance_instances(sign="winding") ----
def test_winding_sign_over_instances(native_lib):
    """a rotated and scaled instance and a mirrored one of a sphere with eight holes, apart: not a mesh the pseudonormal sign is defined
    for (CapPseudonormalsInfo.closed == 0).  Truth: the intact sphere's inside, which every invertible map keeps"""
    whole = unit_sphere()
    tris, holes = punctured(whole, 8)
    rng = np.random.default_rng(9)
    L0 = 1.5 * rotation(rng)
    M = np.stack([affine(L0, (0, 0, 0)), affine(rotation(rng) @ np.diag([1.0, 1.0, -1.0]), (8, 0, 0))])
    qo = (rng.uniform(-1.3, 1.3, (1200, 3))).astype(np.float64)
    # the object-space points farther from every hole than that hole's diameter, and off the facets (test_winding_gpu has the reasons)
    h = holes.astype(np.float64)
    diameter = np.max([np.linalg.norm(h[:, i] - h[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0))], axis=0)
    per_hole = np.stack([np.sqrt(closest(queries(qo.astype(np.float32)), holes[k:k + 1])[0][:, 3].astype(np.float64)) for k in range(len(holes))], 1)
    radius = np.linalg.norm(qo, axis=1)
    clear = (per_hole > 1.5 * diameter[None]).all(1) & ((radius >= 1.01) | (radius <= 0.985))
    assert clear.mean() >= 0.8
    inside = radius[clear] < 0.99
    assert inside.sum() > 100 and (~inside).sum() > 100
    r = context([tris])
    try:
        assert r.build_pseudonormals().closed == 0
        r.set_instances(M)
        with pytest.raises(capi.CapError, match="status 3"):
            r.signed_distance_instances(queries(np.zeros((1, 3), np.float32)), sign="winding")  # needs the dipole table as well
        r.build_winding()
        for i in range(2):
            q = queries((qo[clear] @ M[i, :, 0:3].astype(np.float64).T + M[i, :, 3]).astype(np.float32))
            rec0, inst0, sgn0 = r.signed_distance_instances(q)
            rec, inst, sgn = r.signed_distance_instances(q, sign="winding")
            assert np.array_equal(bits(rec), bits(rec0)) and np.array_equal(inst, inst0), "the records are cap_signed_distance_instances'"
            assert np.array_equal(bits(np.abs(sgn)), bits(np.abs(sgn0))), "and so is the distance"
            assert np.array_equal(sgn < 0, inside), "instance %d: the winding sign is the intact sphere's" % i
        with pytest.raises(capi.CapError, match="mask"):
            r.signed_distance_instances(q, sign="winding", mask=0xFF)
        with pytest.raises(capi.CapError, match="sign must be"):
            r.signed_distance_instances(q, sign="rays")
    finally:
        r.close()
