"""Winding numbers on the GPU (cap_winding_build, cap_winding_numbers): the device's dipole table against the float64 definition on the
read-back tree (winding_support.moments), the query against the host restatement of its walk (winding_support.walk: visit counts bit
for bit, values within a tolerance made of the float32 restatement's own error) and against the float64 brute force, the life cycle
under refit and rebuild, the argument contract, and Renderer.signed_distance(sign="winding")."""
import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import arrays, around, bits, closest, context, queries, sphere
from refit_support import cornell_scene
from signed_distance_support import TRUTH_MESHES, mesh, truth_case, winding_number
from winding_support import (BETAS, OPEN_MESHES, children, child_boxes, moments, octant_triangle, open_cube, overflow_scene, punctured, query_case, unit_sphere, walk, walk32)

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 3
CANARY = 0x7FC0BEEF  # a NaN pattern no winding number and no count holds
R = capi.Renderer
BUILDERS = (R.BVH_BUILD_LBVH, R.BVH_BUILD_PLOC, R.BVH_BUILD_SAH, R.BVH_BUILD_SAH_DEVICE)

# max |walk32 - walk| over each case's kept points and beta = 2, 4, inf, measured on the host on winding_support.median_tree (leaf 4):
# what float32 terms cost against float64 ones.  The device's bound is 8 x this -- the margin covers its atan2f, sqrt and division and
# another tree -- and never below (visits[0] + visits[1]) 2^-24, half an ulp of 1 per term.
MEASURED = {
    "tetrahedron": 1.937e-07, "octahedron": 2.999e-07, "box": 2.428e-06, "torus": 2.041e-07, "sphere": 6.922e-07, "cone": 6.112e-06,
    "open cube": 5.582e-07, "punctured sphere": 7.967e-08, "octant triangle": 2.016e-07,
    "sheared torus": 5.218e-07,  # the moved mesh and the points of the refit test
}
QUERY_CASES = TRUTH_MESHES + tuple(OPEN_MESHES)


def tolerance(name, visits):
    return np.maximum(8.0 * MEASURED[name], visits.sum(1) * 2.0 ** -24)


def raw_call(r, q, beta, with_visits=True, pad=8):
    """cap_winding_numbers on device buffers with canaries behind both outputs: (w float32, visits (N, 2) or None), canaries checked"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(q)
    pts = torch.as_tensor(np.array(q, np.float32), device=dev).contiguous()  # (a copy: the shared points are read-only)
    out = torch.full((n + pad,), CANARY, dtype=torch.int32, device=dev)
    vis = torch.full((n + pad, 2), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = capi.lib().cap_winding_numbers(r.ctx, pts.data_ptr(), n, beta, out.data_ptr(), vis.data_ptr() if with_visits else None)
    assert rc == 0, capi.lib().cap_last_error()
    r.sync()
    o, v = out.cpu().numpy(), vis.cpu().numpy()
    assert (o[n:] == CANARY).all() and (v[n:] == CANARY).all(), "nothing behind the last value or count"
    if not with_visits:
        assert (v == CANARY).all()
    return o[:n].view(np.float32), (v[:n] if with_visits else None)


def assert_table(r, tris, what):
    """the device's table and info against the definition on the device's own tree; returns (nodes, order, table32)"""
    nodes, order = r.bvh_readback()
    info = r.build_winding()
    dev = r.winding_table()
    ref, want = moments(nodes, order, tris)
    assert dev.shape == (max(len(tris) - 1, 0), 2, 8) and len(nodes) == len(dev), what
    assert info.inner_nodes == want["inner_nodes"] and info.degenerate_triangles == want["degenerate_triangles"], what
    assert info.total_area == pytest.approx(want["total_area"], rel=1e-12) and info.ms > 0, what
    A = want["total_area"]
    assert np.abs(np.float64(list(info.root_n)) - want["root_n"]).max() <= 2.0 ** -22 * A, what
    if want["root_p"] is not None:
        assert np.abs(np.float64(list(info.root_p)) - want["root_p"]).max() <= 2.0 ** -22 * np.abs(tris[np.isfinite(tris).all((1, 2))]).max(), what
    if len(dev) == 0:
        return nodes, order, dev
    assert np.array_equal(dev.view(np.int32)[:, :, 7], children(nodes)), "%s: word 7 is the tree's child code, bit for bit" % what
    boxes = child_boxes(nodes).astype(np.float64)
    mag = np.abs(boxes).max((2, 3))
    p, rad, N = dev[:, :, 0:3].astype(np.float64), dev[:, :, 3].astype(np.float64), dev[:, :, 4:7].astype(np.float64)
    assert (np.abs(p - ref[:, :, 0:3]).max(2) <= 2.0 ** -22 * mag).all(), "%s: p~" % what
    assert (np.abs(N - ref[:, :, 4:7]).max(2) <= 2.0 ** -22 * want["areas"]).all(), "%s: N" % what
    far = np.sqrt((np.maximum(np.abs(boxes[:, :, 0] - p), np.abs(boxes[:, :, 1] - p)) ** 2).sum(2))  # from the STORED p~
    assert (rad >= far).all() and (rad <= far * (1 + 2.0 ** -21)).all(), "%s: r covers the box and not much more" % what
    return nodes, order, dev


def assert_query(r, name, tris, pts, tree, betas=BETAS, what=""):
    """visits bit for bit and values within the tolerance of walk on the read-back tree and table; at beta = inf also of the brute force"""
    nodes, order, table = tree
    for beta in betas:
        want, want_visits = walk(nodes, order, tris, table, pts, beta)
        got, visits = raw_call(r, pts, beta)
        assert np.array_equal(visits.astype(np.int64), want_visits), "%s %s beta %s: visits" % (name, what, beta)
        tol = tolerance(name, want_visits)
        err = np.abs(got.astype(np.float64) - want)
        print("%s %s beta %s: max |gpu - walk| %.3e (bound %.3e), mean visits far %.1f exact %.1f" % (
            name, what, beta, err.max(), tol.min(), want_visits[:, 0].mean(), want_visits[:, 1].mean()))
        assert (err <= tol).all(), "%s %s beta %s: %d values off, worst %.3e against %.3e" % (name, what, beta, (err > tol).sum(), err.max(), tol[err.argmax()])
        if np.isinf(beta):
            assert (visits[:, 0] == 0).all() and (visits[:, 1] == len(tris)).all()
            assert (np.abs(got.astype(np.float64) - winding_number(pts, tris)) <= tol).all(), "%s %s: the exact sum against the brute force" % (name, what)
        again, _ = raw_call(r, pts, beta)
        assert np.array_equal(bits(again), bits(got)), "two runs give the same bits"
        plain, _ = raw_call(r, pts, beta, with_visits=False)
        assert np.array_equal(bits(plain), bits(got)), "the same values without the visits array"


# ---- 1. the table ----
def table_scenes():
    degenerate = np.concatenate([np.float32([[(5, 5, 5), (5, 5, 5), (6, 5, 5)]]), mesh("octahedron")[:4], np.float32([[(7, 7, 7), (8, 8, 8), (9, 9, 9)]]),
                                 mesh("octahedron")[4:], np.float32([[(1, 1, 1), (1, 1, 1), (1, 1, 1)]])])
    out = {name: mesh(name) for name in TRUTH_MESHES}
    out.update({name: make() for name, make in OPEN_MESHES.items()})
    out.update({"degenerate triangles": degenerate, "two triangles": mesh("tetrahedron")[:2]})
    return out


@pytest.mark.parametrize("build", BUILDERS)
@pytest.mark.parametrize("name", tuple(table_scenes()))
def test_table_equals_the_definition_on_the_device_tree(native_lib, build, name):
    tris = table_scenes()[name]
    r = context([tris], build)
    try:
        assert_table(r, tris, "%s, builder %d" % (name, build))
        if name == "degenerate triangles":
            assert r.build_winding().degenerate_triangles == 3
        if name == "octant triangle":
            assert r.build_winding().inner_nodes == 0 and r.winding_table().shape == (0, 2, 8), "a root that is a leaf has no records"
    finally:
        r.close()


@pytest.mark.parametrize("build", BUILDERS)
def test_table_of_the_cornell_box(native_lib, cornell_path, build):
    scene, _ = cornell_scene(cornell_path)
    r = capi.Renderer(0)
    try:
        r.set_bvh_build(build)
        r.upload_scene(scene.positions, scene.normals, scene.texcoords, scene.indices, scene.meshes)
        r.build_bvh()
        assert_table(r, scene.triangles(), "Cornell, builder %d" % build)
    finally:
        r.close()


# ---- 2. the query ----
@pytest.mark.parametrize("name", QUERY_CASES)
def test_query_equals_the_walk_and_the_brute_force(native_lib, name):
    tris, pts, _, share = query_case(name)
    assert share >= 0.9
    if len(tris) > 1000:
        pts = pts[::2]  # (the host walk's loop over 4 892 triangles at beta = inf)
    r = context([tris])
    try:
        assert_query(r, name, tris, pts, assert_table(r, tris, name))
    finally:
        r.close()


@pytest.mark.parametrize("build", BUILDERS)
def test_query_on_every_builder(native_lib, build):
    tris, pts, inside, _ = query_case("torus")
    r = context([tris], build)
    try:
        assert_query(r, "torus", tris, pts, assert_table(r, tris, "torus"), what="builder %d" % build)
        w, _ = raw_call(r, pts, 2.0)
        assert np.array_equal(w >= 0.5, inside), "no kept point on the wrong side of 1/2"
    finally:
        r.close()


def test_known_answers(native_lib):
    cases = (("open cube", open_cube(), (0.5, 0.5, 0.5), 5.0 / 6.0), ("octant triangle", octant_triangle(), (0, 0, 0), 0.125),
             ("octant triangle", octant_triangle(flip=True), (0, 0, 0), -0.125))
    for name, tris, at, want in cases:
        r = context([tris])
        try:
            r.build_winding()
            for beta in BETAS:
                w, v = raw_call(r, queries(np.float32([at])), beta)
                assert abs(float(w[0]) - want) <= 8.0 * MEASURED[name], "%s beta %s: %r" % (name, beta, float(w[0]))
                assert v.sum() >= 1
        finally:
            r.close()


def test_far_term_overflow(native_lib):
    """cap_winding_numbers adds a far term as it is: a NaN far term makes the result NaN (cap_winding_instances leaves such a term out;
    test_winding_instances_gpu has the same scene).  Expected: winding_support.walk32 as it stands, visits bit for bit.  Every far term is
    made of correctly rounded operations, so a value made of far terms alone has walk32's bits; an exact term differs from walk32's by
    atan2f alone (2 ulp on the device, numpy's own error, one rounding of the product with 1 / (2 pi): under 5 ulp of a value of at most
    1/2, 5 x 2^-25 < 2^-22 per term)."""
    tris, pts = overflow_scene()
    r = context([tris])
    try:
        r.build_winding()
        nodes, order = r.bvh_readback()
        want, want_visits = walk32(nodes, order, tris, r.winding_table(), pts, 2.0)
        got, visits = raw_call(r, pts, 2.0)
        print("far term overflow: gpu %r visits %r, walk32 %r visits %r" % (got.tolist(), visits.tolist(), want.tolist(), want_visits.tolist()))
        assert want_visits.tolist() == [[2, 0], [2, 0], [0, 2]] and np.isnan(want[0]) and want[1] == 0.0, "the case is what it was built to be"
        assert np.array_equal(visits.astype(np.int64), want_visits)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[0]), "a NaN far term is added: the result is NaN"
        far_only = want_visits[:, 1] == 0
        assert np.array_equal(bits(got[far_only]), bits(want[far_only].astype(np.float32)))
        assert abs(float(got[2]) - want[2]) <= want_visits[2, 1] * 2.0 ** -22
    finally:
        r.close()


def test_python_wrapper(native_lib):
    import torch
    tris, pts, inside, _ = query_case("sphere")
    r = context([tris])
    try:
        with pytest.raises(capi.CapError, match="status 3"):
            r.winding_numbers(pts)
        info = r.build_winding()
        assert info.inner_nodes == len(tris) - 1 and set(info.as_dict()) == {"inner_nodes", "degenerate_triangles", "total_area", "root_n", "root_p", "ms"}
        w, v = r.winding_numbers(pts, visits=True)
        assert isinstance(w, np.ndarray) and w.dtype == np.float32 and v.shape == (len(pts), 2)
        raw, raw_v = raw_call(r, pts, 2.0)
        assert np.array_equal(bits(w), bits(raw)) and np.array_equal(v, raw_v), "beta defaults to 2"
        assert np.array_equal(w >= 0.5, inside)
        dev = torch.as_tensor(pts, device="cuda:0").contiguous()
        out = torch.zeros((len(pts),), dtype=torch.float32, device="cuda:0")
        got = r.winding_numbers(dev, beta=float("inf"), out=out)
        assert got is out and np.abs(out.cpu().numpy() - inside).max() < 1e-4
        with pytest.raises(capi.CapError, match="status 1"):
            r.winding_numbers(pts, beta=0.5)
        r.drop_winding()
        with pytest.raises(capi.CapError, match="status 3"):
            r.winding_table()
    finally:
        r.close()


# ---- 3. refit and rebuild ----
def test_refit_and_rebuild_keep_the_table_current(native_lib):
    tris = mesh("torus")
    P = arrays(tris)[0]
    shear = np.float32([[1.5, 0.0, 0.0], [0.4, 0.75, 0.0], [0.0, -0.3, 2.0]])
    moved = (P @ shear + np.float32([0.25, -1.0, 0.5])).astype(np.float32)
    moved_tris = moved.reshape(-1, 3, 3)
    pts = queries(around(np.random.default_rng(3), moved_tris, 600, 0.3))
    rec, _ = closest(pts, moved_tris)
    v = moved_tris.reshape(-1, 3).astype(np.float64)
    pts = pts[np.sqrt(rec[:, 3].astype(np.float64)) >= 1e-3 * np.linalg.norm(v.max(0) - v.min(0))]
    assert len(pts) >= 540
    r = context([tris], R.BVH_BUILD_SAH_DEVICE)
    try:
        tree = assert_table(r, tris, "built")
        first = r.winding_table()
        # unchanged positions: the refit leaves the bytes as they are
        r.update_vertices(positions=P)
        with pytest.raises(capi.CapError, match="status 3"):
            r.winding_numbers(pts)  # stale
        with pytest.raises(capi.CapError, match="status 3"):
            r.winding_table()
        with pytest.raises(capi.CapError, match="status 3"):
            r.build_winding()
        r.refit_bvh()
        assert np.array_equal(bits(r.winding_table()), bits(first)), "a refit to the same positions gives the same bytes"
        # moved: the refit rebuilds the table on the kept topology
        r.update_vertices(positions=moved)
        r.refit_bvh()
        nodes, order = r.bvh_readback()
        assert np.array_equal(children(nodes), children(tree[0])) and np.array_equal(order, tree[1]), "the topology stays"
        table = r.winding_table()
        assert not np.array_equal(bits(table), bits(first))
        tree = assert_table(r, moved_tris, "after the refit")
        assert np.array_equal(bits(tree[2]), bits(table)), "cap_winding_build after the refit gives the refit's own table"
        assert_query(r, "sheared torus", moved_tris, pts, tree, what="after the refit")
        # another builder: cap_bvh_build rebuilds the table for the new tree
        r.set_bvh_build(R.BVH_BUILD_LBVH)
        r.build_bvh()
        nodes, order = r.bvh_readback()
        assert not np.array_equal(children(nodes), children(tree[0]))
        table = r.winding_table()
        assert np.array_equal(table.view(np.int32)[:, :, 7], children(nodes)), "the table follows the new tree"
        tree = assert_table(r, moved_tris, "after the rebuild")
        assert np.array_equal(bits(tree[2]), bits(table))
        assert_query(r, "sheared torus", moved_tris, pts, tree, betas=(2.0,), what="after the rebuild")
        # masks, instances and objects do not touch it
        r.set_instance_masks([0x00])
        r.set_instances(np.float32([[[1, 0, 0, 5], [0, 1, 0, 0], [0, 0, 1, 0]]]))
        assert np.array_equal(bits(r.winding_table()), bits(table))
        got, _ = raw_call(r, pts, 2.0)
        r.set_instance_masks(None)
        assert np.array_equal(bits(raw_call(r, pts, 2.0)[0]), bits(got)), "a mesh mask is not honoured: the moments cover every triangle"
        # a new scene drops the table
        r.upload_scene(*arrays(tris))
        r.build_bvh()
        with pytest.raises(capi.CapError, match="status 3"):
            r.winding_numbers(pts)
    finally:
        r.close()


# ---- 4. the contract ----
def test_argument_contract(native_lib):
    import torch
    tris, q, _, _ = query_case("torus")
    dev = torch.device("cuda", 0)
    L = capi.lib()
    n = 128
    q = q[:n].copy()
    q[5, 0], q[9, 1], q[17, 2], q[33, 3] = np.nan, np.inf, -np.inf, np.nan  # (the radius is not read)
    pts = torch.as_tensor(q, device=dev).contiguous()
    out = torch.full((n + 8,), CANARY, dtype=torch.int32, device=dev)
    vis = torch.full((n + 8, 2), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    P, O, V = pts.data_ptr(), out.data_ptr(), vis.data_ptr()
    r = capi.Renderer(0)
    try:
        call = lambda p=P, m=n, beta=2.0, o=O, v=V: L.cap_winding_numbers(r.ctx, p, m, beta, o, v)
        r.upload_scene(*arrays(tris))
        assert call() == ERR_STATE and L.cap_winding_build(r.ctx, None) == ERR_STATE and b"cap_bvh_build" in L.cap_last_error()  # before the tree
        r.build_bvh()
        assert call() == ERR_STATE and call(P, 0) == ERR_STATE and b"cap_winding_build" in L.cap_last_error()  # no table: the state comes before n == 0
        assert L.cap_winding_readback(r.ctx, P) == ERR_STATE
        assert L.cap_winding_build(r.ctx, None) == 0  # the info is optional
        assert L.cap_winding_numbers(None, P, n, 2.0, O, V) == ERR_INVALID_ARG
        assert L.cap_winding_build(None, None) == ERR_INVALID_ARG and L.cap_winding_drop(None) == ERR_INVALID_ARG
        assert L.cap_winding_readback(None, None) == ERR_INVALID_ARG and L.cap_winding_readback(r.ctx, None) == ERR_INVALID_ARG
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
        r.sync()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()) and bool((vis == CANARY).all()), "nothing is written on an error"
        assert call(beta=1.0) == 0 and call(beta=float("inf")) == 0 and call() == 0
        r.sync()
        got, gv = out.cpu().numpy(), vis.cpu().numpy()
        assert (got[n:] == CANARY).all() and (gv[n:] == CANARY).all()
        w = got[:n].view(np.float32)
        bad = np.array([5, 9, 17])
        assert np.isnan(w[bad]).all() and (gv[bad] == 0).all(), "a non-finite coordinate: a quiet NaN and visits (0, 0)"
        assert (got[bad] & 0x7FC00000 == 0x7FC00000).all()
        good = np.setdiff1d(np.arange(n), bad)
        nodes, order = r.bvh_readback()
        want, want_visits = walk(nodes, order, tris, r.winding_table(), q, 2.0)
        assert np.array_equal(gv[:n].astype(np.int64), want_visits) and (np.abs(w[good] - want[good]) <= tolerance("torus", want_visits[good])).all()
        assert L.cap_winding_drop(r.ctx) == 0 and call() == ERR_STATE and L.cap_winding_drop(r.ctx) == 0  # drop, then nothing to drop
        with pytest.raises(capi.CapError):
            r.winding_numbers(torch.zeros((4, 3), device=dev))
        with pytest.raises(capi.CapError):
            r.winding_numbers(pts, out=torch.zeros((n, 2), device=dev))
    finally:
        r.close()


def test_a_render_is_unchanged_by_a_table_and_a_query_between_its_batches(native_lib, bluenoise, cornell_path):
    geo = capi.Geometry(cornell_path)
    cam = capi.cornell_camera(64, 64)
    q = queries(np.random.default_rng(5).random((1000, 3)).astype(np.float32) * 600.0 - 20.0)
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
                r.build_winding()
                w = r.winding_numbers(q, beta=float("inf"))
                after = (bits(r.readback(capi.BUF_ACCUM_SUM)), r.stats().as_dict())
                assert np.array_equal(before[0], after[0])
                assert {k: v for k, v in before[1].items() if not k.startswith("ms_")} == {k: v for k, v in after[1].items() if not k.startswith("ms_")}
                P = geo.positions.reshape(-1, 3)
                tris = np.concatenate([P[geo.indices[int(d[3]):int(d[3]) + int(d[2])].astype(np.int64) + int(d[1])].reshape(-1, 3, 3) for d in geo.meshes])
                rec, _ = closest(q, tris)
                off = np.sqrt(rec[:, 3].astype(np.float64)) >= 1e-3 * 600.0
                assert off.mean() >= 0.9
                # float32 terms against float64 ones: a corner minus q is off by an ulp of the coordinates (2^-23 x 560), seen from at
                # least 0.6 away, a handful of such roundings per term, over 2 pi, for each of the triangles
                bound = len(tris) * 4 * 2.0 ** -23 * 560.0 / 0.6 / (2 * np.pi)
                assert np.abs(w - winding_number(q, tris))[off].max() < bound, "the Cornell box (a scene of the exhaustive render path)"
            r.render(2, 2, 2, capi.RENDER_AOV)
            s = r.stats()
            result.append((bits(r.readback(capi.BUF_ACCUM_SUM)), (s.rays_primary, s.rays_extension, s.rays_shadow, s.shaded_vertices, s.frames)))
        finally:
            r.close()
    assert np.array_equal(result[0][0], result[1][0]) and result[0][1] == result[1][1]


# ---- 5. signed_distance(sign="winding") ----
@pytest.mark.parametrize("name", TRUTH_MESHES)
def test_winding_sign_equals_the_pseudonormal_sign_on_closed_meshes(native_lib, name):
    tris = mesh(name)
    q, _, inside, keep = truth_case(name)
    r = context([tris])
    try:
        r.build_pseudonormals()
        with pytest.raises(capi.CapError, match="status 3"):
            r.signed_distance(q, sign="winding")  # needs the dipole table as well
        r.build_winding()
        rec0, sgn0 = r.signed_distance(q)
        rec, sgn = r.signed_distance(q, sign="winding")
        assert np.array_equal(bits(rec), bits(rec0)), "the records are cap_signed_distance's"
        assert np.array_equal(bits(np.abs(sgn)), bits(np.abs(sgn0))), "and so is the distance"
        assert np.array_equal(sgn[keep] < 0, inside) and np.array_equal(sgn0[keep] < 0, inside)
        assert np.array_equal(bits(r.signed_distance(q)[1]), bits(sgn0)), "the default sign is what it was"
        with pytest.raises(capi.CapError, match="mask"):
            r.signed_distance(q, sign="winding", mask=0xFF)
        with pytest.raises(capi.CapError, match="sign must be"):
            r.signed_distance(q, sign="rays")
    finally:
        r.close()


def test_winding_sign_survives_holes(native_lib):
    whole = unit_sphere()
    tris, holes = punctured(whole, 8)
    q = queries(around(np.random.default_rng(9), whole, 2000, 0.3))
    # the points farther from every hole than that hole's diameter (its longest edge), and off the surface by truth_case's rule
    h = holes.astype(np.float64)
    diameter = np.max([np.linalg.norm(h[:, i] - h[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0))], axis=0)
    per_hole = np.stack([np.sqrt(closest(q, holes[k:k + 1])[0][:, 3].astype(np.float64)) for k in range(len(holes))], 1)
    clear = (per_hole > diameter[None]).all(1)
    # the facets of the 50 x 50 sphere lie between the radii 0.996 and 1; 10^-3 of the box diagonal, 3.5e-3, off them
    radius = np.linalg.norm(q[:, 0:3].astype(np.float64), axis=1)
    clear &= (radius >= 1.0035) | (radius <= 0.9925)
    assert clear.mean() >= 0.9
    truth = np.round(winding_number(q[clear], whole)).astype(int) == 1  # the intact sphere's
    assert truth.sum() > 100 and (~truth).sum() > 100
    r = context([tris])
    try:
        pn = r.build_pseudonormals()
        assert pn.closed == 0 and pn.boundary_edges >= 24, "not a mesh the pseudonormal sign is defined for"
        r.build_winding()
        _, sgn = r.signed_distance(q, sign="winding")
        assert np.array_equal(sgn[clear] < 0, truth)
    finally:
        r.close()
