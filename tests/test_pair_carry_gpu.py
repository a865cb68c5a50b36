"""Candidate mask of the fused small-scene kernels of bounce >= 1 by POSITION (csrc/cap_exhaustive.h): in a scene made of fan pairs
only, pair j holding triangles 2j and 2j + 1, the list is walked from its last triangle to its first and every triangle shifts its
inside bit in with one carry-chain step, one word up to 32 triangles, two up to 64.  Every other scene keeps the id-indexed loop.
Each case renders through the public interface, compares the four planes and the three ray counters bit for bit with the oracle,
and asks cap_debug_get(CAP_DEBUG_MARK_FORM) which form the launches took, so that a fallback cannot pass for the new loop.  The
shapes are the smallest at which the insertion can go wrong: 2 triangles, an odd pair count (the tail step), bits 0 and 31, bits 32
and 63 (the carry between the words), exact ties, a ray inside both triangles of a pair, idle lanes at a class's end, signed zeros
in d.n and in the records.  (A library built with -DCAP_MARK_V1, CAP_LIB_VARIANT=markv1, must report the id-indexed loop throughout.)"""
import os

import numpy as np
import pytest

from capsaicin_amd import capi

pytestmark = pytest.mark.gpu

PLANES = (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("direct", capi.BUF_DIRECT), ("indirect", capi.BUF_INDIRECT),
          ("normal_depth", capi.BUF_NORMAL_DEPTH))
BY_ID, CARRY, CARRY2 = 1, 2, 3
MARK_V1 = os.environ.get("CAP_LIB_VARIANT") == "markv1"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, ref, name):
    g, r = bits(got), bits(ref)
    if not np.array_equal(g, r):
        bad = np.argwhere((g != r).any(-1))
        msg = ["%s: %d pixels differ" % (name, len(bad))]
        for b in bad[:6]:
            msg.append("  (y,x)=%s gpu=%s oracle=%s" % (tuple(b), got[tuple(b)], ref[tuple(b)]))
        raise AssertionError("\n".join(msg))


def one_mesh(nverts, nidx):
    return np.uint32([[nverts, 0, nidx, 0, 0, 0xFFFFFFFF, 0, 0]])


def finish(verts, idx, seed=0, nrm=None):
    pos = np.float32(verts)
    idx = np.uint32(idx)
    if nrm is None:
        tri = pos[np.int64(idx)].reshape(-1, 3, 3)
        fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-12)
        nrm = np.zeros_like(pos)
        nrm[np.int64(idx)] = np.repeat(fn, 3, axis=0)
    uv = np.random.RandomState(seed).rand(len(pos), 2).astype(np.float32)
    return pos, np.float32(nrm), uv, idx, one_mesh(len(pos), len(idx))


def soup(seed, order, fold):
    """order: 'q' = a quad triangulated as the fan (a,b,c),(a,c,d), 's' = a loose triangle, in the order given; fold > 0 lifts the
    fourth vertex out of the plane of the first three, so a ray can be inside both triangles of a pair"""
    rs = np.random.RandomState(seed)
    verts, idx = [], []
    for kind in order:
        c = rs.uniform(-1.5, 1.5, 3)
        u, v = rs.normal(size=3), rs.normal(size=3)
        u, v = 0.9 * u / np.linalg.norm(u), 0.9 * v / np.linalg.norm(v)
        base = len(verts)
        if kind == "q":
            n = np.cross(u, v)
            verts += [c, c + u, c + u + v + fold * n / max(np.linalg.norm(n), 1e-6) * rs.uniform(-1, 1), c + v]
            idx += [base, base + 1, base + 2, base, base + 2, base + 3]
        else:
            verts += [c, c + u, c + v]
            idx += [base, base + 1, base + 2]
    return finish(verts, idx, seed)


def shuffled(seed, nquads, nsingles):
    order = ["q"] * nquads + ["s"] * nsingles
    np.random.RandomState(seed).shuffle(order)
    return "".join(order)


def stack(zs, half=1.2):
    """parallel quads at the given z, vertex normals (0, 0, -1): bounce rays leave the front quads towards -z through the others"""
    verts, idx = [], []
    for z in zs:
        base = len(verts)
        verts += [(-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)]
        idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return finish(verts, idx, nrm=np.tile(np.float32([0, 0, -1]), (len(verts), 1)))


def tunnel(nstack, z0):
    """nstack quads at z0 + 0.2 k, then four bit-identical copies at z0 + 0.2 nstack: nearest to the camera, highest ids"""
    return stack([np.float32(z0 + 0.2 * k) for k in range(nstack)] + [np.float32(z0 + 0.2 * nstack)] * 4)


def zero_box():
    """Axis-aligned room (five faces, open towards the camera) with a partition in the plane x = -0.0 that the camera lies in, seen by
    an axis-aligned camera: tvec.n is +0 or -0 for every camera ray against the partition, two of the three products of every d.n are
    signed zeros, and the records hold -0.0 coordinates and normals like the Cornell box's `vn -0 1 0`."""
    z = np.float32(-0.0)
    faces = [  # (corners, normal)
        ([(-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1)], (z, 1, z)),    # floor
        ([(-1, 1, 1), (1, 1, 1), (1, 1, -1), (-1, 1, -1)], (z, -1, z)),       # ceiling
        ([(-1, -1, -1), (-1, 1, -1), (1, 1, -1), (1, -1, -1)], (z, z, 1)),    # back wall
        ([(-1, -1, 1), (-1, 1, 1), (-1, 1, -1), (-1, -1, -1)], (1, z, z)),    # left wall
        ([(1, -1, -1), (1, 1, -1), (1, 1, 1), (1, -1, 1)], (-1, z, z)),       # right wall
        ([(z, -1, -0.5), (z, 0.25, -0.5), (z, 0.25, 0.5), (z, -1, 0.5)], (1, z, z)),  # partition in the camera's plane
    ]
    verts, idx, nrm = [], [], []
    for corners, n in faces:
        base = len(verts)
        verts += corners
        nrm += [n] * 4
        idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return finish(verts, idx, nrm=np.float32(nrm))


def camera(w, h, position=(0.2, 0.1, 6.0)):
    cam = capi.CameraData()
    cam.position[:] = position
    cam.forward[:] = (0, 0, -1)
    cam.right[:] = (-1, 0, 0)
    cam.up[:] = (0, 1, 0)
    cam.focal_length = 0.03
    cam.sensor_size[0] = 0.036
    cam.sensor_size[1] = np.float32(0.036) * (np.float32(h) / np.float32(w))
    return cam


def expected_form(dense, ntri):
    if MARK_V1 or not dense:
        return BY_ID
    return CARRY2 if ntri > 32 else CARRY


def run_case(bluenoise, scene, w, h, frames, depth, dense, materials=None, check=None, cam=None, geometry=None):
    """scene: the five arrays; geometry: a capi.Geometry to upload instead (the same scene from its file)"""
    from oracle import cap_oracle as O
    pos, nrm, uv, idx, meshes = scene
    ntri = len(idx) // 3
    assert ntri <= 64  # the fused kernels with the scene in LDS
    cam = cam or camera(w, h)
    ext = materials is not None
    sc = O.Scene(pos, nrm, uv, idx, meshes, materials=materials) if ext else O.Scene(pos, nrm, uv, idx, meshes)
    ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1], cam.focal_length)
    r = capi.Renderer(0)
    if geometry is not None:
        r.upload_geometry(geometry)
    else:
        r.upload_scene(pos, nrm, uv, idx, meshes)
    if ext:
        r.upload_materials(materials)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(w, h)
    r.set_camera(cam)
    assert r.debug_get(r.DEBUG_MARK_FORM) == (1 if dense else 0)  # the scene's own property; no launch yet
    for frame in frames:
        ref = sc.render_frame(ocam, bluenoise, w, h, frame, depth, flags=O.FLAG_EXT_MATERIALS if ext else 0, threads=8)
        prim = bits(ref["gbuffer_geo"])[..., 3]
        hits = int((prim != 0xFFFFFFFF).sum())
        print("frame", frame, "oracle rays", ref["rays"], "camera hits", hits)
        assert ref["rays"][1] > 0.05 * w * h  # the camera sees the scene and paths go on
        if check:
            check(ref, prim, hits)
        r.stats_reset()
        r.render(frame, 1, depth, capi.RENDER_AOV | (capi.RENDER_EXT_MATERIALS if ext else 0))  # AUTO: at most 64 triangles -> fused kernels
        for name, kind in PLANES:
            assert_same(r.readback(kind), ref[name], name)
        s = r.stats()
        assert (s.rays_primary, s.rays_extension, s.rays_shadow) == ref["rays"]
        got = r.debug_get(r.DEBUG_MARK_FORM)
        print("mark form", got >> 8, "dense", got & 1)
        assert got & 0xff == (1 if dense else 0)
        assert got >> 8 == expected_form(dense, ntri)
    r.close()


def test_one_quad_under_a_sky(native_lib, bluenoise):
    """2 triangles: the whole word but bits 0 and 1 stays empty"""
    run_case(bluenoise, stack([np.float32(0.0)]), 16, 8, (5,), 3, dense=True)


def test_three_quads_tail_step(native_lib, bluenoise):
    """an odd pair count: the last pair is taken alone, first"""
    run_case(bluenoise, stack([np.float32(-0.4), np.float32(-0.2), np.float32(0.0)]), 24, 16, (5, 6), 3, dense=True)


def tie_check(lowest):
    def check(ref, prim, hits):
        on_lowest = int((prim == lowest).sum())
        print("pixels on the lowest coincident id", on_lowest)
        assert ref["rays"][1] >= 2 * hits  # paths go on through the stack
        assert on_lowest > 0               # the coincident copies are what the camera sees, and the tie went to the lowest id
        assert int((prim != 0xFFFFFFFF).sum() - (prim == lowest).sum() - (prim == lowest + 1).sum()) == 0
    return check


def test_tunnel_32_triangles(native_lib, bluenoise):
    """16 quads: bits 0 and 31 in use, the last four quads bit-equal (ties go to the lower id), lanes with up to 32 candidates"""
    scene = tunnel(12, -1.0)
    assert len(scene[3]) // 3 == 32
    run_case(bluenoise, scene, 24, 16, (5,), 4, dense=True, check=tie_check(24))


def test_folded_soup_without_singles(native_lib, bluenoise):
    """a ray inside both triangles of a pair: both bits of one asm statement set in one lane"""
    scene = soup(35, "q" * 15, 0.6)
    run_case(bluenoise, scene, 24, 16, (5, 6), 3, dense=True)


@pytest.mark.parametrize("w,h", [(16, 8), (100, 52)])
def test_cornell_box(native_lib, bluenoise, cornell_path, w, h):
    """the headline scene (32 triangles, `vn -0 1 0` normals); 100 x 52: partial tiles and idle lanes at a class's end (has_ray)"""
    from oracle import obj_oracle
    g = obj_oracle.load_geometry(cornell_path)
    scene = (g["positions"], g["normals"], g["texcoords"], g["indices"], g["meshes"])
    assert len(scene[3]) // 3 == 32
    run_case(bluenoise, scene, w, h, (0, 1), 8, dense=True, cam=capi.cornell_camera(w, h), geometry=capi.Geometry(cornell_path))


def test_two_words_carry_crosses(native_lib, bluenoise):
    """17 quads = 34 triangles: bits 32 and 33 are reached through the low word's carry-out"""
    scene = tunnel(13, -1.2)
    assert len(scene[3]) // 3 == 34
    run_case(bluenoise, scene, 24, 16, (5,), 4, dense=True, check=tie_check(26))


def test_two_words_bit_63(native_lib, bluenoise):
    """32 quads = 64 triangles: every bit of both words"""
    scene = tunnel(28, -4.0)
    assert len(scene[3]) // 3 == 64
    run_case(bluenoise, scene, 24, 16, (5,), 4, dense=True, check=tie_check(56))


def test_two_words_folded_soup(native_lib, bluenoise):
    scene = soup(36, "q" * 30, 0.4)
    run_case(bluenoise, scene, 24, 16, (5,), 3, dense=True)


def test_signed_zeros(native_lib, bluenoise):
    scene = zero_box()
    assert np.signbit(scene[0]).any() and np.signbit(scene[1][scene[1] == 0]).any()  # -0.0 coordinates and normals went in
    run_case(bluenoise, scene, 24, 16, (5, 6), 3, dense=True, cam=camera(24, 16, position=(0.0, 0.0, 3.0)))


@pytest.mark.parametrize("order", [shuffled(32, 14, 4), "s" + "q" * 15, "q" * 15 + "s"])
def test_scenes_that_are_not_dense(native_lib, bluenoise, order):
    """loose triangles shuffled in; one loose triangle first, so every pair's id is odd; one last: the id-indexed loop, same bits"""
    run_case(bluenoise, soup(32, order, 0.0), 24, 16, (5,), 3, dense=False)


def test_ext_instantiation(native_lib, bluenoise):
    """The EXT model's bounce >= 1 kernel calls the same function: 16 planar quads (dense), the last two emissive (next-event rays)."""
    pos, nrm, uv, idx, _ = soup(31, "q" * 16, 0.0)
    meshes = np.uint32([[56, 0, 84, 0, 0, 0xFFFFFFFF, 0, 0], [8, 56, 12, 84, 1, 0xFFFFFFFF, 0, 0]])
    idx = idx.copy()
    idx[84:] -= 56
    mats = np.zeros((2, 12), np.float32)
    mats[0, 0:3], mats[0, 3], mats[0, 4:7] = (0.7, 0.6, 0.5), 0.4, (0.04, 0.04, 0.04)
    mats[1, 0:3], mats[1, 3], mats[1, 8:11] = (0.5, 0.5, 0.5), 1.0, (12.0, 11.0, 8.0)

    def check(ref, prim, hits):
        assert ref["rays"][2] > 0  # next-event rays were cast

    run_case(bluenoise, (pos, nrm, uv, idx, meshes), 24, 16, (5,), 4, dense=True, materials=mats, check=check)
