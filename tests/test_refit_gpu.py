"""Vertex updates and in-place refit (cap_scene_update_vertices / cap_bvh_refit) on the MI355X.  Trees and records are compared on raw
uint32 bits: an identity refit reproduces every builder's trees byte for byte; queries and renders on a moved, refitted scene equal
the oracle's brute force and a second context that uploaded the moved arrays and built; boxes stay conservative under large motion;
device and host sources agree; and the state contract holds."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from refit_support import (Scene, assert_same_render, assert_same_trees, bits, check_binary_conservative, check_brute_force,
                           check_wide_conservative, context, cornell_scene, expected_node_visits, hall_camera, hall_scene, rays_into,
                           render_result, trees)

pytestmark = pytest.mark.gpu
BUILDERS = (0, 1, 2, 3, 4)
ERR_INVALID_ARG, ERR_STATE = 1, 3


@pytest.fixture(scope="module")
def cornell(cornell_path):
    return cornell_scene(cornell_path)


@pytest.fixture(scope="module")
def hall():
    s = hall_scene(1.0)
    assert len(s.indices) // 3 > 250000
    return s


def rotate_one_shear_rest(scene):
    """Cornell: the mesh with the most triangles below the ceiling (a box) turns about y, the rest shears in x by y"""
    P = scene.positions.astype(np.float64).copy()
    vm = scene.vertex_mesh()
    counts = [int(d[2]) // 3 for d in scene.meshes]
    m = int(np.argmax(counts))
    sel = vm == m
    c = P[sel].mean(0)
    a = 0.4
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    P[sel] = (P[sel] - c) @ R.T + c
    P[~sel, 0] += 0.07 * P[~sel, 1]
    return P.astype(np.float32)


def wave(scene, t, translate_mesh=3, amount=0.05):
    """the hall: a smooth displacement along y, one mesh translated"""
    P = scene.positions.astype(np.float64).copy()
    P[:, 1] += amount * np.sin(0.7 * P[:, 0] + 0.3 * P[:, 2] + t)
    sel = scene.vertex_mesh() == translate_mesh
    P[sel] += np.array([0.3 * np.sin(t), 0.1, 0.2])
    return P.astype(np.float32)


def refit_to(r, positions):
    r.update_vertices(positions=positions)
    return r.refit_bvh()


# ---- 1. identity refit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cornell", "hall"])
@pytest.mark.parametrize("build", BUILDERS)
def test_identity_refit_reproduces_the_build(native_lib, cornell, hall, which, build):
    scene = cornell[0] if which == "cornell" else hall
    r = context(scene, build)
    before = trees(r)
    info = refit_to(r, scene.positions)
    assert_same_trees(before, trees(r), "after an identity refit (builder %d, %s)" % (build, which))
    assert info.expected_node_visits == info.expected_node_visits_built
    np.testing.assert_allclose(info.expected_node_visits, expected_node_visits(before[0].view(np.float32)), rtol=1e-12)
    assert info.ms > 0
    r.close()


@pytest.mark.parametrize("which", ["cornell", "hall"])
def test_identity_refit_host_collapse(native_lib, cornell, hall, which):
    scene = cornell[0] if which == "cornell" else hall
    r = context(scene, 3, host_collapse=True)
    before = trees(r)
    refit_to(r, scene.positions)
    assert_same_trees(before, trees(r), "after an identity refit of the host collapse")
    r.close()


# ---- 2. deform, then restore -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDERS)
def test_deform_then_restore(native_lib, hall, build):
    r = context(hall, build)
    before = trees(r)
    info = refit_to(r, wave(hall, 1.0, amount=0.3))
    assert info.expected_node_visits != info.expected_node_visits_built
    refit_to(r, hall.positions)
    assert_same_trees(before, trees(r), "after deform + restore (builder %d)" % build)
    r.close()


# ---- 3. queries on a moved scene -------------------------------------------------------------------------------------------------
def _queries_match(r, moved, rays, all_triangles, build=None):
    rec = r.trace_rays(rays)
    occ = r.trace_occlusion(rays)
    tris = moved.triangles()
    check_brute_force(rays, rec, tris, all_triangles)
    fresh = context(moved, build)
    assert np.array_equal(bits(rec), bits(fresh.trace_rays(rays))), "refitted tree and fresh build disagree"
    assert np.array_equal(occ, fresh.trace_occlusion(rays))
    fresh.close()
    # the binary-tree kernels on the refitted tree
    r.debug_switch("CAP_NO_WIDE8", 1)
    assert np.array_equal(bits(rec), bits(r.trace_rays(rays))), "wide and binary kernels disagree on the refitted tree"
    assert np.array_equal(occ, r.trace_occlusion(rays))
    r.debug_switch("CAP_NO_WIDE8", 0)
    # occlusion agrees with the closest hit: hits well inside (tmin, tmax) occlude, unbounded rays that miss do not
    m = 1e-5
    t, g = rec[:, 0].astype(np.float64), bits(rec)[:, 3]
    tmin, tmax = rays[:, 3].astype(np.float64), rays[:, 7].astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = (g != capi.MISS) & (t > tmin + m * (1 + np.abs(t))) & (t < tmax - m * (1 + np.abs(t)))
    assert np.all(occ[inside] == 1) and inside.sum() > len(rays) // 4
    assert np.all(occ[(g == capi.MISS) & np.isinf(tmax)] == 0)


def test_queries_cornell_moved(native_lib, cornell):
    scene = cornell[0]
    moved = scene.moved(positions=rotate_one_shear_rest(scene))
    r = context(scene)
    refit_to(r, moved.positions)
    rays = rays_into(moved.triangles(), np.random.default_rng(3), 3000)
    _queries_match(r, moved, rays, True)
    r.close()


@pytest.mark.parametrize("build", [0, 2])
def test_queries_hall_moved(native_lib, hall, build):
    moved = hall.moved(positions=wave(hall, 0.5))
    r = context(hall, build)
    refit_to(r, moved.positions)
    rays = rays_into(moved.triangles(), np.random.default_rng(5), 600)
    _queries_match(r, moved, rays, False, build)
    r.close()


# ---- 4. renders on a moved scene -------------------------------------------------------------------------------------------------
def test_render_cornell_small_scene_path(native_lib, bluenoise, cornell):
    scene, _ = cornell
    moved = scene.moved(positions=rotate_one_shear_rest(scene))
    cam = capi.cornell_camera(80, 60)
    r = context(scene, bluenoise=bluenoise)
    refit_to(r, moved.positions)
    a = render_result(r, cam, 80, 60, 2, 3)
    f = context(moved, bluenoise=bluenoise)
    assert_same_render(a, render_result(f, cam, 80, 60, 2, 3), "(Cornell, fan-pair path)")
    r.close(), f.close()


def test_render_cornell_ext_lamp_moved(native_lib, bluenoise, cornell):
    scene, mats = cornell
    emissive = [m for m in range(len(mats)) if mats[m, 8:11].max() > 0] if mats.shape[1] > 10 else []
    lamp = emissive[0] if emissive else int(np.argmax([int(d[2]) for d in scene.meshes]))
    P = scene.positions.copy()
    sel = scene.vertex_mesh() == lamp
    P[sel] += np.array([0.1, -0.05, 0.08], np.float32)
    moved = scene.moved(positions=P)
    cam = capi.cornell_camera(80, 60)
    r = context(scene, bluenoise=bluenoise, materials=mats)
    refit_to(r, moved.positions)
    a = render_result(r, cam, 80, 60, 2, 3, capi.RENDER_AOV | capi.RENDER_EXT_MATERIALS)
    nee_a = r.debug_get(capi.Renderer.DEBUG_NEE_PAIRS) if hasattr(capi.Renderer, "DEBUG_NEE_PAIRS") else None
    f = context(moved, bluenoise=bluenoise, materials=mats)
    b = render_result(f, cam, 80, 60, 2, 3, capi.RENDER_AOV | capi.RENDER_EXT_MATERIALS)
    assert_same_render(a, b, "(Cornell, EXT, lamp moved)")
    if nee_a is not None:
        assert nee_a == f.debug_get(capi.Renderer.DEBUG_NEE_PAIRS)
    r.close(), f.close()


def test_render_hall_tree_path_two_lanes(native_lib, bluenoise, hall):
    moved = hall.moved(positions=wave(hall, 2.0))
    w, h = 64, 48
    cam = hall_camera(w, h)
    r = context(hall, bluenoise=bluenoise)
    refit_to(r, moved.positions)
    a = render_result(r, cam, w, h, 4, 2, batch_paths=w * h)
    assert r.debug_get(capi.Renderer.DEBUG_LANES_USED) == 2
    f = context(moved, bluenoise=bluenoise)
    assert_same_render(a, render_result(f, cam, w, h, 4, 2, batch_paths=w * h), "(hall, two lanes)")
    r.close(), f.close()


# ---- 5. large motion -------------------------------------------------------------------------------------------------------------
def test_large_motion_keeps_boxes_conservative(native_lib, hall):
    P = hall.positions.astype(np.float64).copy()
    vm = hall.vertex_mesh()
    lo, hi = P.min(0), P.max(0)
    ext = hi - lo
    rng = np.random.default_rng(11)
    for m in range(len(hall.meshes)):
        P[vm == m] += (rng.random(3) - 0.5) * 9.0 * ext
    moved = hall.moved(positions=P.astype(np.float32))
    r = context(hall)
    info = refit_to(r, moved.positions)
    nlo, nhi = moved.positions.min(0), moved.positions.max(0)
    assert np.max(nhi - nlo) > 5.0 * np.max(ext)
    assert info.expected_node_visits > info.expected_node_visits_built
    nodes, leaves, wn, src, _, _ = trees(r)
    tris = moved.triangles()
    check_binary_conservative(nodes, leaves, tris)
    check_wide_conservative(wn, src, leaves, tris)
    bi = r.bvh_info()
    assert np.array_equal(np.float32(bi.bounds_lo[:]), nlo) and np.array_equal(np.float32(bi.bounds_hi[:]), nhi)
    rays = rays_into(tris, np.random.default_rng(13), 400)
    check_brute_force(rays, r.trace_rays(rays), tris)
    r.close()


# ---- 6. device and host sources --------------------------------------------------------------------------------------------------
def test_device_and_host_sources_agree(native_lib, hall):
    import torch
    moved = wave(hall, 0.25)
    a, b = context(hall), context(hall)
    a.update_vertices(positions=moved)
    ia = a.refit_bvh()
    t = torch.from_numpy(moved).to("cuda:0") * 1.0  # written on torch's stream
    b.update_vertices(positions=t)
    ib = b.refit_bvh()
    assert_same_trees(trees(a), trees(b), "(device vs host source)")
    assert ia.expected_node_visits == ib.expected_node_visits
    rays = rays_into(hall.triangles(moved), np.random.default_rng(17), 2000)
    assert np.array_equal(bits(a.trace_rays(rays)), bits(b.trace_rays(rays)))
    a.close(), b.close()


def test_normals_and_uvs_only_update(native_lib, bluenoise, cornell):
    import torch
    scene, _ = cornell
    rng = np.random.default_rng(19)
    N = scene.normals + rng.normal(scale=0.2, size=scene.normals.shape).astype(np.float32)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    T = (scene.texcoords * 1.5 + 0.25).astype(np.float32)
    cam = capi.cornell_camera(80, 60)
    r = context(scene, bluenoise=bluenoise)
    r.update_vertices(normals=torch.from_numpy(N).to("cuda:0"), texcoords=torch.from_numpy(T).to("cuda:0"))
    r.refit_bvh()
    f = context(scene.moved(normals=N, texcoords=T), bluenoise=bluenoise)
    assert_same_render(render_result(r, cam, 80, 60, 2, 3), render_result(f, cam, 80, 60, 2, 3), "(normals / uvs only)")
    r.close(), f.close()


# ---- 7. state contract -----------------------------------------------------------------------------------------------------------
def test_state_contract(native_lib, bluenoise, cornell):
    import torch
    scene, _ = cornell
    L = native_lib
    r = capi.Renderer(0)
    r.upload_scene(scene.positions, scene.normals, scene.texcoords, scene.indices, scene.meshes)
    assert L.cap_bvh_refit(r.ctx, None) == ERR_STATE  # no tree yet
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(32, 24)
    r.set_camera(capi.cornell_camera(32, 24))
    p = np.ascontiguousarray(scene.positions)
    pv = p.ctypes.data_as(ctypes.c_void_p)
    assert L.cap_scene_update_vertices(r.ctx, pv, None, None, 2) == ERR_INVALID_ARG  # unknown flag
    assert L.cap_scene_update_vertices(r.ctx, pv, None, None, capi.VERTICES_DEVICE) == ERR_INVALID_ARG  # host memory as device
    dt = torch.from_numpy(p).to("cuda:0")
    mis = ctypes.c_void_p(dt.data_ptr() + 2)
    assert L.cap_scene_update_vertices(r.ctx, mis, None, None, capi.VERTICES_DEVICE) == ERR_INVALID_ARG  # misaligned
    r.render(0, 1, 1)  # (the failed calls changed nothing)
    r.sync()
    assert L.cap_scene_update_vertices(r.ctx, pv, None, None, 0) == 0
    rays = torch.zeros((4, 8), device="cuda:0")
    hits = torch.zeros((4, 4), device="cuda:0")
    occ = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    buf = np.zeros(64 * 16, np.float32)
    assert L.cap_render(r.ctx, 0, 1, 1, 0) == ERR_STATE
    assert L.cap_trace_rays(r.ctx, ctypes.c_void_p(rays.data_ptr()), 4, ctypes.c_void_p(hits.data_ptr()), 0) == ERR_STATE
    assert L.cap_trace_occlusion(r.ctx, ctypes.c_void_p(rays.data_ptr()), 4, ctypes.c_void_p(occ.data_ptr()), 0) == ERR_STATE
    assert L.cap_bvh_readback(r.ctx, buf.ctypes.data_as(ctypes.c_void_p), None) == ERR_STATE
    info = np.zeros(3, np.uint32)
    assert L.cap_bvh_wide_readback(r.ctx, None, None, info.ctypes.data_as(ctypes.c_void_p)) == ERR_STATE
    r.refit_bvh()
    r.render(0, 1, 1)
    r.sync()
    # a new scene clears the refit state
    r.upload_scene(scene.positions, scene.normals, scene.texcoords, scene.indices, scene.meshes)
    assert L.cap_bvh_refit(r.ctx, None) == ERR_STATE
    r.close()


def test_build_after_update_equals_fresh(native_lib, hall):
    moved = hall.moved(positions=wave(hall, 0.75))
    r = context(hall, 4)
    r.update_vertices(positions=moved.positions)
    r.build_bvh()
    f = context(moved, 4)
    assert_same_trees(trees(r), trees(f), "(build after an update)")
    r.close(), f.close()


def test_one_triangle_scene_moves(native_lib):
    tri = Scene(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.tile([[0, 0, 1]], (3, 1)), np.zeros((3, 2)),
                np.array([0, 1, 2], np.uint32), np.array([[3, 0, 3, 0, 0, 0, 0, 0]], np.uint32))
    r = context(tri)
    before = trees(r)
    refit_to(r, tri.positions)
    assert_same_trees(before, trees(r), "(one triangle, identity)")
    moved = tri.positions + np.array([5.0, -3.0, 2.0], np.float32)
    refit_to(r, moved)
    ray = np.array([[5.25, -2.75, 10.0, 0.0, 0.0, 0.0, -1.0, np.inf], [0.25, 0.25, 10.0, 0.0, 0.0, 0.0, -1.0, np.inf]], np.float32)
    rec = r.trace_rays(ray)
    assert bits(rec)[0, 3] == 0 and abs(float(rec[0, 0]) - 8.0) < 1e-5  # hit where it went ...
    assert bits(rec)[1, 3] == capi.MISS                                    # ... and not where it was
    check_brute_force(ray, rec, tri.triangles(moved), True)
    f = context(tri.moved(positions=moved))
    assert_same_trees(trees(r), trees(f), "(one triangle moved)")
    r.close(), f.close()


def test_two_contexts_refit_alike(native_lib, hall):
    moved = wave(hall, 1.5)
    a, b = context(hall), context(hall)
    refit_to(a, moved), refit_to(b, moved)
    assert_same_trees(trees(a), trees(b), "(two contexts)")
    a.close(), b.close()


# ---- 8. a sequence ---------------------------------------------------------------------------------------------------------------
def test_animated_sequence(native_lib, bluenoise, hall):
    w, h = 48, 32
    cam = hall_camera(w, h)
    r = context(hall, bluenoise=bluenoise)
    r.set_resolution(w, h)
    r.set_camera(cam)
    for f in range(30):
        P = wave(hall, 0.1 * f)
        r.update_vertices(positions=P)
        r.refit_bvh()
        r.render(f, 1, 2, capi.RENDER_AOV)
    last = render_result(r, cam, w, h, 1, 2)
    fresh = context(hall.moved(positions=P), bluenoise=bluenoise)
    assert_same_render(last, render_result(fresh, cam, w, h, 1, 2), "(frame 30 of a sequence)")
    r.close(), fresh.close()
