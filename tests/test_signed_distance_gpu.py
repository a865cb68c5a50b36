"""Signed distance on the GPU (cap_pseudonormals_build, cap_signed_distance): the device's table against the float64 reference of
signed_distance_support.py, the weld across four ways of uploading one triangle list, the query bit for bit -- records against
cap_closest_points, signs against the float32 reference run on the device's read-back table --, the signs against the float64 winding
number, masks, the life cycle and the argument contract."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import MISS, arrays, around, assert_records, bits, closest, context, queries, sphere
from signed_distance_support import (MESHES, TRUTH_MESHES, assert_table, box, indexed, indexed_arrays, mesh, octahedron, pseudonormals, reference_table,
                                     signed_distance, signed_of, stats_of, tetrahedron, truth_case)

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 3
CANARY = 0x7FC0BEEF  # a NaN pattern no record and no distance holds
B = capi.Renderer  # the CapBvhBuild values
INF_BITS = 0x7F800000


def assert_signed(got, want, what=""):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, "%s: %d of %d signed distances differ, first %d: got %r want %r" % (what, len(bad), len(g), bad[0], float(np.ravel(got)[bad[0]]),
                                                                                             float(np.ravel(want)[bad[0]]))


def raw_call(r, q, pad=8, options=None):
    """cap_signed_distance on device buffers with canaries behind both outputs: (records, signed) as numpy, canaries checked"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(q)
    pts = torch.as_tensor(np.ascontiguousarray(q, np.float32), device=dev).contiguous()
    out = torch.full((n + pad, 8), CANARY, dtype=torch.int32, device=dev)
    sgn = torch.full((n + pad,), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = capi.lib().cap_signed_distance(r.ctx, pts.data_ptr(), n, out.data_ptr(), sgn.data_ptr(), options)
    assert rc == 0, capi.lib().cap_last_error()
    r.sync()
    o, s = out.cpu().numpy().view(np.float32), sgn.cpu().numpy().view(np.float32)
    assert (bits(o[n:]) == CANARY).all() and (bits(s[n:]) == CANARY).all(), "nothing behind the last record or distance"
    return o[:n], s[:n]


# ---- 1. the table ----
def defect_scenes():
    tet = tetrahedron()
    flipped = tet.copy()
    flipped[3] = flipped[3][[0, 2, 1]]
    fins = np.float32([[(0, 0, 0), (0, 0, 1), (1, 0, 0)], [(0, 0, 0), (0, 0, 1), (0, 1, 0)], [(0, 0, 0), (0, 0, 1), (-1, -1, 0)]])
    # (two corners at one position, three on a line, all three at one position; a non-finite corner is left to the CPU reference: no
    # builder of the tree is tested on one)
    bad = np.concatenate([np.float32([[(5, 5, 5), (5, 5, 5), (6, 5, 5)]]), tet[:2], np.float32([[(7, 7, 7), (8, 8, 8), (9, 9, 9)]]), tet[2:],
                          np.float32([[(1, 1, 1), (1, 1, 1), (1, 1, 1)]]), np.float32([[(0, -0.0, 2), (0, 0, 2), (3, 3, 3)]])])
    return {"one face removed": tet[:3], "one face flipped": flipped, "three triangles on one edge": fins, "degenerate triangles": bad,
            "one triangle": tet[:1]}


@pytest.mark.parametrize("name", tuple(MESHES) + tuple(defect_scenes()))
def test_table_and_statistics_equal_the_float64_reference(native_lib, name):
    if name in MESHES:
        tris, (ref, stats) = mesh(name), reference_table(name)
    else:
        tris = defect_scenes()[name]
        ref, stats = pseudonormals(tris)
    r = context([tris])
    try:
        info = r.build_pseudonormals()
        assert stats_of(info) == stats, name
        dev = r.pseudonormals()
        assert dev.shape == (len(tris), 7, 3) and dev.dtype == np.float32
        assert_table(dev, ref, name)
        assert (dev[(ref == 0).all(2)] == 0).all(), "an entry that is zero in the reference is exactly zero"
        if name == "degenerate triangles":
            assert stats["degenerate_triangles"] == 4 and stats["closed"] == 1 and stats["vertices"] == 4
            for g in (0, 3, 6, 7):
                assert (bits(dev[g]) == 0).all(), "all seven entries of a degenerate triangle are +0"
    finally:
        r.close()


# ---- 2. the weld ----
def test_four_ways_to_upload_one_triangle_list_give_one_table(native_lib):
    tris = np.concatenate([sphere(12, 12), octahedron() * np.float32(0.25) + np.float32([3, 0, 0]), octahedron()])
    ref, stats = pseudonormals(tris)
    half = len(tris) // 2
    negative = tris.copy()
    zero = np.argwhere(negative == 0)
    assert len(zero) > 40
    for g, k, j in zero[::2]:  # every other zero coordinate: copies of one vertex now differ in the sign of a zero
        negative[g, k, j] = np.float32(-0.0)
    assert np.signbit(negative).sum() > np.signbit(tris).sum() + 20
    uploads = {
        "soup": arrays(tris),
        "one indexed mesh": indexed_arrays(indexed(tris)),
        "two meshes, soup and indexed": indexed_arrays((tris[:half].reshape(-1, 3), np.arange(3 * half)), indexed(tris[half:])),
        "some zeros negative": arrays(negative),
    }
    assert len(uploads["one indexed mesh"][0]) < len(uploads["soup"][0]) // 3
    tables = {}
    for name, a in uploads.items():
        r = capi.Renderer(0)
        try:
            r.upload_scene(*a)
            r.build_bvh()
            assert stats_of(r.build_pseudonormals()) == stats, name
            tables[name] = r.pseudonormals()
        finally:
            r.close()
    assert_table(tables["soup"], ref, "soup")
    for name, t in tables.items():
        assert np.array_equal(bits(t), bits(tables["soup"])), name


# ---- 3. the query, bit for bit ----
def query_set(name, n=4097):
    """n points in and around the mesh: unbounded, a quarter with radii that split into hits and misses, degenerate ones in between"""
    tris = mesh(name)
    rng = np.random.default_rng(11)
    q = queries(around(rng, tris, n, 0.5))
    ext = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    q[n // 2::2, 3] = rng.random(len(q[n // 2::2])).astype(np.float32) * np.float32(0.3 * ext)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for k, (col, value) in enumerate(((0, nan), (1, inf), (2, -inf), (3, np.float32(-1.0)), (3, nan))):
        q[5 + 7 * k::97, col] = value
    return q


_expected = {}


def expected(name):
    """the brute-force records of query_set(name), once"""
    if name not in _expected:
        q = query_set(name)
        _expected[name] = (q, closest(q, mesh(name))[0])
    return _expected[name]


@pytest.mark.parametrize("build", (B.BVH_BUILD_LBVH, B.BVH_BUILD_SAH_DEVICE), ids=("lbvh", "sah_device"))
@pytest.mark.parametrize("name", tuple(MESHES))
def test_records_and_signs_bit_for_bit(native_lib, name, build):
    tris = mesh(name)
    q, want = expected(name)
    hit = bits(want)[:, 6] != MISS
    assert 0.6 * len(q) < hit.sum() < len(q) - 100, "hits and misses"
    r = context([tris], build)
    try:
        r.build_pseudonormals()
        table = r.pseudonormals()
        want_signed = signed_of(want, q, tris, table)
        assert (want_signed[hit] < 0).sum() > 20 and (want_signed[hit] > 0).sum() > 20 and (bits(want_signed[~hit]) == INF_BITS).all()
        for n in (1, 63, 64, 65, 4097):
            rec, sgn = raw_call(r, q[:n])
            assert_records(rec, want[:n], "%s, n = %d" % (name, n))
            assert_records(rec, r.closest_points(q[:n]), "%s, n = %d against cap_closest_points" % (name, n))
            assert_signed(sgn, want_signed[:n], "%s, n = %d" % (name, n))
        rec, sgn = r.signed_distance(q)
        assert_records(rec, want, name + ", the wrapper")
        assert_signed(sgn, want_signed, name + ", the wrapper")
    finally:
        r.close()


@pytest.mark.parametrize("name", ("box", "octahedron"))
def test_points_on_vertices_edges_and_faces_give_plus_zero(native_lib, name):
    tris = mesh(name)
    t = tris.astype(np.float64)
    pts = np.concatenate([t.reshape(-1, 3), 0.5 * (t[:, 0] + t[:, 1]), 0.5 * (t[:, 1] + t[:, 2]), 0.25 * (2 * t[:, 0] + t[:, 1] + t[:, 2])])
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts), "exact in binary32"
    q = queries(pts.astype(np.float32))
    want, _ = closest(q, tris)
    assert (want[:, 3] == 0).all() and len(set(bits(want)[:, 7].tolist())) >= 5, "computed dist2 0 on vertices, edges and faces"
    r = context([tris])
    try:
        r.build_pseudonormals()
        rec, sgn = raw_call(r, q)
        assert_records(rec, want, name)
        assert (bits(sgn) == 0).all(), "+0.0, not -0.0"
    finally:
        r.close()


# ---- 4. truth ----
@pytest.mark.parametrize("name", TRUTH_MESHES)
def test_no_wrong_sign_against_the_winding_number(native_lib, name):
    q, want, inside, keep = truth_case(name)
    r = context([mesh(name)])
    try:
        r.build_pseudonormals()
        rec, sgn = r.signed_distance(q.copy())
        assert_records(rec, want, name)
        wrong = int(((sgn[keep] < 0) != inside).sum())
        print("%s: %d kept, %d inside, %d wrong signs" % (name, len(keep), inside.sum(), wrong))
        assert np.isfinite(sgn).all() and wrong == 0
    finally:
        r.close()


# ---- 5. masks ----
def test_masks_select_the_candidates_and_leave_the_table(native_lib):
    a, b = box(), box((2.0, 1.0, 1.0), 0b101010, (4.0, 0.5, 0.25))
    tris = np.concatenate([a, b])
    rng = np.random.default_rng(5)
    q = queries(around(rng, tris, 2048, 0.3))
    in_a = np.arange(len(tris)) < len(a)
    r = context([a, b])
    try:
        r.build_pseudonormals()
        table = r.pseudonormals()
        assert_table(table, pseudonormals(tris)[0], "two boxes")
        r.set_instance_masks([0x01, 0x02])
        assert np.array_equal(bits(r.pseudonormals()), bits(table)), "the masks do not touch the table"
        for mask, sel in ((0x01, in_a), (0x02, ~in_a), (0x03, None), (None, None)):
            want, want_signed = signed_distance(q, tris, table, sel)
            rec, sgn = r.signed_distance(q, mask=mask)
            assert_records(rec, want, "mask %r" % mask)
            assert_records(rec, r.closest_points(q, mask=mask), "mask %r against cap_closest_points" % mask)
            assert_signed(sgn, want_signed, "mask %r" % mask)
            assert (sgn < 0).sum() > 10
        rec, sgn = r.signed_distance(q, mask=0xFC)
        assert (bits(rec)[:, 6] == MISS).all() and (bits(sgn) == INF_BITS).all(), "a mask nothing passes"
        r.set_instance_masks([0x00, 0xFF])
        want, want_signed = signed_distance(q, tris, table, ~in_a)
        rec, sgn = r.signed_distance(q)
        assert_records(rec, want, "a mesh with mask 0")
        assert_signed(sgn, want_signed, "a mesh with mask 0")
        assert np.array_equal(bits(r.pseudonormals()), bits(table))
    finally:
        r.close()


# ---- 6. life cycle ----
def test_life_cycle(native_lib):
    tris = sphere(12, 12)
    P = arrays(tris)[0]
    moved = (P * np.float32([1.5, 0.75, 2.0]) + np.float32([0.25, -1.0, 0.5])).astype(np.float32)
    moved_tris = moved.reshape(-1, 3, 3)
    rng = np.random.default_rng(3)
    q = queries(around(rng, moved_tris, 512, 0.3))
    L = capi.lib()
    state = lambda: pytest.raises(capi.CapError, match="status 3")
    r = capi.Renderer(0)
    try:
        r.upload_scene(*arrays(tris))
        with state():
            r.build_pseudonormals()  # before the tree
        r.build_bvh()
        with state():
            r.signed_distance(q)  # without a table
        with state():
            r.pseudonormals()
        assert b"cap_pseudonormals_build" in L.cap_last_error()
        info = r.build_pseudonormals()
        assert stats_of(info) == pseudonormals(tris)[1] and info.ms > 0 and info.closed == 0 and info.boundary_edges == 24
        assert L.cap_pseudonormals_build(r.ctx, None) == 0  # the info is optional
        first = r.pseudonormals()
        want, want_signed = signed_distance(q, tris, first)
        rec, sgn = r.signed_distance(q)
        assert_records(rec, want, "built")
        assert_signed(sgn, want_signed, "built")
        r.drop_pseudonormals()
        with state():
            r.signed_distance(q)  # after drop
        r.drop_pseudonormals()  # nothing to drop: fine
        r.build_pseudonormals()
        assert np.array_equal(bits(r.pseudonormals()), bits(first))
        # stale, then current again after a refit and after a rebuild
        r.update_vertices(positions=moved)
        with state():
            r.signed_distance(q)
        with state():
            r.pseudonormals()
        with state():
            r.build_pseudonormals()
        ref_moved, stats_moved = pseudonormals(moved_tris)
        # the move rounds the south pole's vertices, 1e-16 apart before, onto one position: the rebuild has to weld again
        assert stats_moved["closed"] == 1 and stats_moved["vertices"] == info.vertices - 11
        for step in ("refit", "build"):
            r.refit_bvh() if step == "refit" else r.build_bvh()
            table = r.pseudonormals()
            assert_table(table, ref_moved, "after the " + step)
            assert stats_of(r.build_pseudonormals()) == stats_moved and np.array_equal(bits(r.pseudonormals()), bits(table))
            assert not np.array_equal(bits(table), bits(first))
            want, want_signed = signed_distance(q, moved_tris, table)
            rec, sgn = r.signed_distance(q)
            assert_records(rec, want, "after the " + step)
            assert_signed(sgn, want_signed, "after the " + step)
            assert (sgn < 0).sum() > 20 and (sgn > 0).sum() > 20
            r.update_vertices(positions=moved)  # (stale again for the next step)
        r.build_bvh()
        # a new scene drops the table
        r.upload_scene(*arrays(tris))
        r.build_bvh()
        with state():
            r.signed_distance(q)
        with state():
            r.pseudonormals()
    finally:
        r.close()


# ---- 7. arguments ----
def test_argument_contract(native_lib):
    import torch
    tris = mesh("torus")
    dev = torch.device("cuda", 0)
    L = capi.lib()
    n = 128
    q = query_set("torus", 256)[:n]
    pts = torch.as_tensor(q, device=dev).contiguous()
    out = torch.full((n + 8, 8), CANARY, dtype=torch.int32, device=dev)
    sgn = torch.full((n + 8,), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    P, O, S = pts.data_ptr(), out.data_ptr(), sgn.data_ptr()
    r = context([tris])
    try:
        call = lambda p=P, m=n, o=O, s=S, opt=None: L.cap_signed_distance(r.ctx, p, m, o, s, opt)
        assert call() == ERR_STATE and call(P, 0) == ERR_STATE  # no table: the state comes before n == 0
        r.build_pseudonormals()
        assert L.cap_signed_distance(None, P, n, O, S, None) == ERR_INVALID_ARG
        assert L.cap_pseudonormals_build(None, None) == ERR_INVALID_ARG and L.cap_pseudonormals_drop(None) == ERR_INVALID_ARG
        assert L.cap_pseudonormals_readback(None, None) == ERR_INVALID_ARG and L.cap_pseudonormals_readback(r.ctx, None) == ERR_INVALID_ARG
        assert call(None) == ERR_INVALID_ARG and call(P, n, None) == ERR_INVALID_ARG and call(P, n, O, None) == ERR_INVALID_ARG and b"NULL" in L.cap_last_error()
        assert call(P + 4) == ERR_INVALID_ARG and b"points is not 16-byte aligned" in L.cap_last_error()
        assert call(P, n, O + 8) == ERR_INVALID_ARG and b"output is not 16-byte aligned" in L.cap_last_error()
        assert call(P, n, O, S + 2) == ERR_INVALID_ARG and b"signed is not 4-byte aligned" in L.cap_last_error()
        assert call(P, n, P) == ERR_INVALID_ARG and b"points and output ranges overlap" in L.cap_last_error()
        assert call(P, n, O, P + 16 * (n - 1)) == ERR_INVALID_ARG and b"points and signed ranges overlap" in L.cap_last_error()
        assert call(P, n, O, O + 32 * (n - 1) + 28) == ERR_INVALID_ARG and b"output and signed ranges overlap" in L.cap_last_error()
        assert call(S, n // 8, O) == ERR_INVALID_ARG and call(P, 1 << 60) == ERR_INVALID_ARG and b"address space" in L.cap_last_error()
        option = lambda *o: ctypes.byref(capi.TraceOptions(o[0], o[1], (ctypes.c_uint32 * 2)(*o[2:])))
        for flags in (0x04, 0x10, 0x20, 0x01, 0x80000000):
            assert call(opt=option(flags, 0, 0, 0)) == ERR_INVALID_ARG and b"ray_flags" in L.cap_last_error()
        assert call(opt=option(0, 0, 1, 0)) == ERR_INVALID_ARG and call(opt=option(0, 0x100, 0, 0)) == ERR_INVALID_ARG
        assert call(None, 0, None, None) == 0  # nothing to do
        r.sync()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()) and bool((sgn == CANARY).all()), "nothing is written on an error"
        assert call(opt=option(0, 0, 0, 0)) == 0  # the all-zero options are the plain call
        r.sync()
        want, want_signed = signed_distance(q, tris, r.pseudonormals())
        got, gs = out.view(torch.float32).cpu().numpy(), sgn.view(torch.float32).cpu().numpy()
        assert_records(got[:n], want, "the call itself")
        assert_signed(gs[:n], want_signed, "the call itself")
        assert (bits(got[n:]) == CANARY).all() and (bits(gs[n:]) == CANARY).all()
        with pytest.raises(capi.CapError):
            r.signed_distance(torch.zeros((4, 3), device=dev))
        with pytest.raises(capi.CapError):
            r.signed_distance(pts, out=torch.zeros((n, 4), device=dev))
    finally:
        r.close()


def test_a_render_is_unchanged_by_a_table_and_a_query_between_its_batches(native_lib, bluenoise, cornell_path):
    geo = capi.Geometry(cornell_path)
    cam = capi.cornell_camera(64, 64)
    rng = np.random.default_rng(5)
    q = queries(rng.random((1000, 3)).astype(np.float32) * 600.0 - 20.0)
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
                r.build_pseudonormals()
                rec, sgn = r.signed_distance(q)
                after = (bits(r.readback(capi.BUF_ACCUM_SUM)), r.stats().as_dict())
                assert np.array_equal(before[0], after[0])
                assert {k: v for k, v in before[1].items() if not k.startswith("ms_")} == {k: v for k, v in after[1].items() if not k.startswith("ms_")}
                P = geo.positions.reshape(-1, 3)
                tris = np.concatenate([P[geo.indices[int(d[3]):int(d[3]) + int(d[2])].astype(np.int64) + int(d[1])].reshape(-1, 3, 3) for d in geo.meshes])
                table = r.pseudonormals()
                want, want_signed = signed_distance(q, tris, table)
                assert_records(rec, want, "the Cornell box (a scene of the exhaustive render path)")
                assert_signed(sgn, want_signed, "the Cornell box")
            r.render(2, 2, 2, capi.RENDER_AOV)
            s = r.stats()
            result.append((bits(r.readback(capi.BUF_ACCUM_SUM)), (s.rays_primary, s.rays_extension, s.rays_shadow, s.shaded_vertices, s.frames)))
        finally:
            r.close()
    assert np.array_equal(result[0][0], result[1][0]) and result[0][1] == result[1][1]
