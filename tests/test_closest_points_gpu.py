"""Closest-point queries on the GPU (cap_closest_points): every record compared bit for bit, all eight words, with the numpy float32
brute force of closest_point_support.py over every triangle."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import (MISS, arrays, around, assert_records, bits, closest, context, near_surface, needles, queries, soup, sphere)
from multi_hit_support import stacked_quads

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 3
CANARY = 0x7FC0BEEF  # a NaN pattern no record holds
B = capi.Renderer  # the CapBvhBuild values


def run(r, q, mask=None):
    return r.closest_points(np.ascontiguousarray(q, np.float32), mask=mask)


@pytest.fixture(scope="module")
def soup_case():
    """5 000 small triangles (above the AUTO builder's threshold of 4 096) and 2 048 points inside and outside their box, half of them
    with a finite radius; the brute force, once"""
    rng = np.random.default_rng(7)
    tris = soup(rng, 5000, edge=0.05)
    q = queries(around(rng, tris, 2048, 0.5))
    q[1024:, 3] = rng.random(1024).astype(np.float32) * 0.2
    want, table = closest(q, tris)
    return tris, q, want, table


# 1. ties
def tie_points(n_quads, dz):
    z_mid = (np.arange(n_quads - 1) + 0.5) * dz
    out = []
    for z in z_mid[::3]:
        out += [(0.5, 0.25, z), (0.25, 0.5, z), (0.5, 0.5, z), (0.25, 0.25, z), (0.75, 0.75, z), (0, 0, z), (1, 1, z), (1, 0, z), (0, 1, z), (2, 2, z), (-1, 0.5, z)]
    out += [(0.5, 0.5, -3.0), (40.0, -30.0, 100.0), (0.5, 0.25, n_quads * dz + 5.0), (0.25, 0.25, 0.0), (1.0, 1.0, dz)]
    return queries(out)


@pytest.mark.parametrize("doubled", (False, True), ids=("quads", "every triangle twice"))
def test_ties_go_to_the_lower_id(native_lib, doubled):
    _, tris = stacked_quads(40, 0.25)
    if doubled:
        tris = np.concatenate([tris, tris])
    q = tie_points(40, 0.25)
    want, table = closest(q, tris)
    # the expected set really holds ties that the higher id would have lost
    winners = bits(want)[:, 6].astype(np.int64)
    tied = (table == table[np.arange(len(q)), winners][:, None]).sum(1)
    assert (winners != MISS).all() and (tied >= 2).sum() > 0.9 * len(q) and (tied >= 4).sum() > 10
    if doubled:
        assert (winners < 80).all() and (tied >= 2).all()
    r = context([tris])
    try:
        assert_records(run(r, q), want, "ties")
    finally:
        r.close()


# 2. builders
@pytest.mark.parametrize("build", (B.BVH_BUILD_LBVH, B.BVH_BUILD_SAH, B.BVH_BUILD_PLOC, B.BVH_BUILD_SAH_DEVICE, B.BVH_BUILD_AUTO),
                         ids=("lbvh", "sah", "ploc", "sah_device", "auto"))
def test_every_builder_equals_the_brute_force(native_lib, soup_case, build):
    tris, q, want, _ = soup_case
    hit = bits(want)[:, 6] != MISS
    assert hit[:1024].all() and 100 < hit[1024:].sum() < 1000, "the radii split the second half into hits and misses"
    r = context([tris], build)
    try:
        assert_records(run(r, q), want, "builder %d" % build)
    finally:
        r.close()


# 3. scenes built against the prune
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
    want, _ = closest(q, tris)
    assert (bits(want)[:, 6] != MISS).all()
    r = context([tris])
    try:
        assert_records(run(r, q), want, name)
        # the same with the radius a hair above the answer's distance: the bound starts thin instead of becoming so
        q2 = q.copy()
        q2[:, 3] = np.sqrt(want[:, 3]) * np.float32(1.000001)
        want2, _ = closest(q2, tris)
        assert_records(run(r, q2), want2, name + ", tight radius")
    finally:
        r.close()


def test_points_on_vertices_and_edges_with_radius_zero(native_lib, soup_case):
    tris = soup_case[0]
    _, quads = stacked_quads(8, 0.25)
    scene = np.concatenate([tris + np.float32([2, 0, 0]), quads])
    on_vertices = scene[::7].reshape(-1, 3)
    z = np.arange(8) * 0.25
    on_edges = np.concatenate([[(0.5, 0, k), (1, 0.5, k), (0.5, 0.5, k), (0, 0.25, k), (0.75, 1, k)] for k in z])
    q = queries(np.concatenate([on_vertices, on_edges]), 0.0)
    off = q.copy()
    off[:, 2] += np.float32(1e-3)  # ... and just off them: radius 0 admits nothing
    q = np.concatenate([q, off])
    want, _ = closest(q, scene)
    n = len(q) // 2
    assert (bits(want)[:n, 6] != MISS).all() and (want[:n, 3] == 0).all(), "a point on a vertex or an exact edge has computed dist2 0"
    assert (bits(want)[n:, 6] == MISS).sum() > 0.9 * n and (want[n:, 3] == 0).all()
    r = context([scene])
    try:
        assert_records(run(r, q), want, "radius 0")
    finally:
        r.close()


# 4. radius
def test_radius_at_one_ulp_below_and_without(native_lib, soup_case):
    tris, q, _, table = soup_case
    q = q[:512].copy()
    best = table[:512].min(1)
    at = np.sqrt(best)
    assert at.dtype == np.float32
    below = np.nextafter(at, np.float32(0))
    r = context([tris])
    try:
        hits = {}
        for name, radius in (("at", at), ("below", below), ("inf", np.float32(np.inf))):
            q[:, 3] = radius
            want, _ = closest(q, tris)
            hits[name] = bits(want)[:, 6] != MISS
            assert (want[~hits[name], 3] == q[~hits[name], 3] * q[~hits[name], 3]).all(), "the miss record carries r2"
            assert_records(run(r, q), want, "radius " + name)
        # sqrt rounds either way: fl(r * r) lands on both sides of dist2
        assert hits["inf"].all() and 50 < hits["at"].sum() < 512 and hits["below"].sum() < hits["at"].sum()
    finally:
        r.close()


# 5. degenerate queries
def test_degenerate_queries_between_good_ones(native_lib, soup_case):
    import torch
    tris, q, _, _ = soup_case
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    q = q[:96].copy()
    for k, (col, value) in enumerate(((0, nan), (1, inf), (2, -inf), (3, np.float32(-1.0)), (3, nan), (3, -inf), (0, -nan), (1, nan))):
        q[1 + 3 * k::24, col] = value
    want, _ = closest(q, tris)
    bad = ~np.isfinite(q[:, 0:3]).all(1) | ~(q[:, 3] >= 0)
    assert bad.sum() == 32
    miss = np.zeros(8, np.uint32)
    miss[6] = MISS
    assert (bits(want)[bad] == miss).all() and (bits(want)[~bad, 6] != MISS).sum() > 20
    dev = torch.device("cuda", 0)
    out = torch.full((len(q) + 4, 8), CANARY, dtype=torch.int32, device=dev).view(torch.float32)
    r = context([tris])
    try:
        r.closest_points(torch.as_tensor(q, device=dev), out=out[:len(q)])
        got = out.cpu().numpy()
        assert_records(got[:len(q)], want, "degenerate queries")
        assert (bits(got[len(q):]) == CANARY).all()
    finally:
        r.close()


# 6. sizes, and the smallest trees
@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_sizes_with_canaries(native_lib, soup_case, n):
    import torch
    tris, q, want, _ = soup_case
    reps = -(-n // len(q))
    qn, wn = np.tile(q, (reps, 1))[:n], np.tile(want, (reps, 1))[:n]
    dev = torch.device("cuda", 0)
    out = torch.full((n + 8, 8), CANARY, dtype=torch.int32, device=dev).view(torch.float32)
    r = context([tris])
    try:
        r.closest_points(torch.as_tensor(qn, device=dev), out=out[:n])
        got = out.cpu().numpy()
        assert_records(got[:n], wn, "n = %d" % n)
        assert (bits(got[n:]) == CANARY).all(), "nothing behind the last record"
    finally:
        r.close()


@pytest.mark.parametrize("count", (1, 2, 3))
def test_smallest_scenes(native_lib, soup_case, count):
    """one triangle (the root is a leaf), two (one node, one traversal leaf) and three"""
    tris, q, _, _ = soup_case
    few = tris[:count]
    q = q[:256].copy()
    q[128:, 3] = 0.6
    want, _ = closest(q, few)
    hit = bits(want)[:, 6] != MISS
    assert hit[:128].all() and 0 < hit[128:].sum() < 128
    r = context([few])
    try:
        assert r.bvh_info().triangle_count == count
        assert_records(run(r, q), want, "%d triangles" % count)
    finally:
        r.close()


# 7. masks
def test_masks_and_option_errors(native_lib, soup_case):
    import torch
    tris, q, want_all, _ = soup_case
    q = q[:512]
    a, b = tris[:2500], tris[2500:]
    in_a = np.arange(len(tris)) < 2500
    want_a, _ = closest(q, tris, in_a)
    want_b, _ = closest(q, tris, ~in_a)
    assert not np.array_equal(bits(want_a), bits(want_b)) and (bits(want_b)[:, 6][bits(want_b)[:, 6] != MISS] >= 2500).all()
    dev = torch.device("cuda", 0)
    r = context([a, b])
    try:
        assert_records(run(r, q), want_all[:512], "two meshes, no table")
        r.set_instance_masks([0x01, 0x02])
        assert_records(run(r, q), want_all[:512], "plain call, both masks non-zero")
        assert_records(run(r, q, mask=0x01), want_a, "mask 1")
        assert_records(run(r, q, mask=0x02), want_b, "mask 2")
        assert_records(run(r, q, mask=0x03), want_all[:512], "mask 3")
        assert_records(run(r, q, mask=0xFC), closest(q, tris, np.zeros(len(tris), bool))[0], "a mask nothing passes")
        r.set_instance_masks([0x00, 0xFF])
        assert_records(run(r, q), want_b, "a mesh with mask 0 is invisible to the plain call")
        r.set_instance_masks(None)
        assert_records(run(r, q, mask=0x01), want_all[:512], "no table: every mesh passes every mask")

        # options the call refuses: nothing is written
        L = capi.lib()
        pts = torch.as_tensor(q, device=dev).contiguous()
        out = torch.full((len(q), 8), CANARY, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        call = lambda *o: L.cap_closest_points(r.ctx, pts.data_ptr(), len(q), out.data_ptr(), ctypes.byref(capi.TraceOptions(o[0], o[1], (ctypes.c_uint32 * 2)(*o[2:]))))
        for flags in (0x04, 0x10, 0x20, 0x01, 0x80000000):
            assert call(flags, 0, 0, 0) == ERR_INVALID_ARG and b"ray_flags" in L.cap_last_error()
        assert call(0, 0, 1, 0) == ERR_INVALID_ARG and call(0, 0, 0, 7) == ERR_INVALID_ARG and b"reserved" in L.cap_last_error()
        assert call(0, 0x100, 0, 0) == ERR_INVALID_ARG and call(0, 0xFFFFFFFF, 0, 0) == ERR_INVALID_ARG
        r.sync()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all())
        assert call(0, 0, 0, 0) == 0  # the all-zero options are the plain call
        r.sync()
        assert_records(out.view(torch.float32).cpu().numpy(), want_all[:512], "all-zero options")
        with pytest.raises(capi.CapError):
            r.closest_points(q, mask=0x100)
    finally:
        r.close()


# 8. refit
def test_stale_until_refit_then_the_moved_vertices(native_lib, soup_case):
    tris, q, want, _ = soup_case
    q = q[:512]
    rng = np.random.default_rng(3)
    P = arrays(tris)[0]
    moved = (P + np.float32([0.05, -0.02, 0.03]) + (rng.random(P.shape) - 0.5).astype(np.float32) * np.float32(0.02)).astype(np.float32)
    want_moved, _ = closest(q, moved.reshape(-1, 3, 3))
    assert not np.array_equal(bits(want_moved), bits(want[:512]))
    r = context([tris])
    try:
        assert_records(run(r, q), want[:512], "before the update")
        r.update_vertices(positions=moved)
        with pytest.raises(capi.CapError, match="status 3.*cap_bvh_refit"):
            run(r, q)
        r.refit_bvh()
        assert_records(run(r, q), want_moved, "after the refit")
        r.build_bvh()
        assert_records(run(r, q), want_moved, "after a rebuild")
    finally:
        r.close()


# 9. errors and state
def test_argument_and_state_contract(native_lib, soup_case):
    import torch
    tris, q, want, _ = soup_case
    dev = torch.device("cuda", 0)
    L = capi.lib()
    n = 128
    pts = torch.as_tensor(q[:n], device=dev).contiguous()
    out = torch.full((n + 8, 8), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    P, O = pts.data_ptr(), out.data_ptr()
    r = capi.Renderer(0)
    try:
        call = lambda p=P, m=n, o=O: L.cap_closest_points(r.ctx, p, m, o, None)
        assert call() == ERR_STATE and b"cap_bvh_build" in L.cap_last_error()  # nothing uploaded
        r.upload_scene(*arrays(tris))
        assert call() == ERR_STATE and call(P, 0) == ERR_STATE  # uploaded, not built: the state comes before n == 0
        r.build_bvh()
        assert L.cap_closest_points(None, P, n, O, None) == ERR_INVALID_ARG
        assert call(None) == ERR_INVALID_ARG and call(P, n, None) == ERR_INVALID_ARG and b"NULL" in L.cap_last_error()
        assert call(P + 4) == ERR_INVALID_ARG and b"points is not 16-byte aligned" in L.cap_last_error()
        assert call(P, n, O + 8) == ERR_INVALID_ARG and b"output is not 16-byte aligned" in L.cap_last_error()
        assert call(P, n, P) == ERR_INVALID_ARG and call(P, n, P + 16 * (n - 1)) == ERR_INVALID_ARG and b"overlap" in L.cap_last_error()
        assert call(O + 32 * (n - 1), n, O) == ERR_INVALID_ARG
        assert call(P, 1 << 60) == ERR_INVALID_ARG and b"address space" in L.cap_last_error()
        assert call(None, 0, None) == 0  # nothing to do
        r.sync()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()), "nothing is written on an error"
        assert call() == 0
        r.sync()
        got = out.view(torch.float32).cpu().numpy()
        assert_records(got[:n], want[:n], "the call itself")
        assert (bits(got[n:]) == CANARY).all()
        with pytest.raises(capi.CapError):
            r.closest_points(torch.zeros((4, 3), device=dev))
        with pytest.raises(capi.CapError):
            r.closest_points(pts, out=torch.zeros((n, 4), device=dev))
    finally:
        r.close()


def test_a_render_is_unchanged_by_a_query_between_its_batches(native_lib, bluenoise, cornell_path):
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
                rec = r.closest_points(q)
                after = (bits(r.readback(capi.BUF_ACCUM_SUM)), r.stats().as_dict())
                assert np.array_equal(before[0], after[0])
                assert {k: v for k, v in before[1].items() if not k.startswith("ms_")} == {k: v for k, v in after[1].items() if not k.startswith("ms_")}
                P = geo.positions.reshape(-1, 3)
                tris = np.concatenate([P[geo.indices[int(d[3]):int(d[3]) + int(d[2])].astype(np.int64) + int(d[1])].reshape(-1, 3, 3) for d in geo.meshes])
                assert_records(rec, closest(q, tris)[0], "the Cornell box (a scene of the exhaustive render path)")
            r.render(2, 2, 2, capi.RENDER_AOV)
            s = r.stats()
            result.append((bits(r.readback(capi.BUF_ACCUM_SUM)), (s.rays_primary, s.rays_extension, s.rays_shadow, s.shaded_vertices, s.frames)))
        finally:
            r.close()
    assert np.array_equal(result[0][0], result[1][0]) and result[0][1] == result[1][1]
