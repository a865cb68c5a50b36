"""Two-phase closest hit of the fused small-scene kernels (bounce >= 1 of scenes of at most 64 triangles): phase 1 marks, per lane,
the triangles the ray's line passes inside of as bits indexed by global triangle id (one word up to 32 triangles, two up to 64);
phase 2 computes t for the marked ones in ascending id order with a strict compare.  The shapes are the smallest at which that
can go wrong -- bit 31 and bit 63 in use, ids of pairs and loose triangles interleaved, a ray inside both triangles of a folded
quad, lanes with up to 32 / 64 candidates whose winner has a high id, bit-equal coincident quads (ties go to the lower id), idle
lanes of partial tiles, the EXT model's instantiation -- each compared bit for bit with the oracle's brute force."""
import numpy as np
import pytest

from capsaicin_amd import capi

pytestmark = pytest.mark.gpu

PLANES = (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("direct", capi.BUF_DIRECT), ("indirect", capi.BUF_INDIRECT),
          ("normal_depth", capi.BUF_NORMAL_DEPTH))


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


def fan_soup(seed, nquads, nsingles, fold):
    """Quads triangulated as fans (a,b,c),(a,c,d), loose triangles shuffled in between; fold > 0 lifts the fourth vertex out of
    the plane of the first three, so a ray can be inside both triangles of a pair.  Returns per-face vertex blocks too."""
    rs = np.random.RandomState(seed)
    verts, idx = [], []
    order = ["q"] * nquads + ["s"] * nsingles
    rs.shuffle(order)
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
    pos = np.float32(verts)
    tri = pos[np.int64(idx)].reshape(-1, 3, 3)
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-12)
    nrm = np.zeros_like(pos)
    nrm[np.int64(idx)] = np.repeat(fn, 3, axis=0)
    uv = rs.rand(len(pos), 2).astype(np.float32)
    return pos, nrm.astype(np.float32), uv, np.uint32(idx), one_mesh(len(pos), len(idx))


def tunnel(nstack, z0):
    """nstack parallel quads +-1.2 wide at z = z0 + 0.2 k, then four bit-identical copies at z0 + 0.2 nstack, vertex normals
    (0, 0, -1): bounce rays leave the front quads towards -z through the whole stack."""
    zs = [np.float32(z0 + 0.2 * k) for k in range(nstack)] + [np.float32(z0 + 0.2 * nstack)] * 4
    verts, idx = [], []
    for z in zs:
        base = len(verts)
        verts += [(-1.2, -1.2, z), (1.2, -1.2, z), (1.2, 1.2, z), (-1.2, 1.2, z)]
        idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    pos = np.float32(verts)
    nrm = np.tile(np.float32([0, 0, -1]), (len(pos), 1))
    uv = np.tile(np.float32([[0, 0], [1, 0], [1, 1], [0, 1]]), (len(zs), 1))
    return pos, nrm, uv, np.uint32(idx), one_mesh(len(pos), len(idx))


def camera(w, h):
    cam = capi.CameraData()
    cam.position[:] = (0.2, 0.1, 6.0)
    cam.forward[:] = (0, 0, -1)
    cam.right[:] = (-1, 0, 0)
    cam.up[:] = (0, 1, 0)
    cam.focal_length = 0.03
    cam.sensor_size[0] = 0.036
    cam.sensor_size[1] = np.float32(0.036) * (np.float32(h) / np.float32(w))
    return cam


def run_case(bluenoise, scene, w, h, frame, depth, materials=None, check=None):
    from oracle import cap_oracle as O
    pos, nrm, uv, idx, meshes = scene
    ntri = len(idx) // 3
    assert ntri <= 64  # the fused kernels with the scene in LDS
    cam = camera(w, h)
    ext = materials is not None
    sc = O.Scene(pos, nrm, uv, idx, meshes, materials=materials) if ext else O.Scene(pos, nrm, uv, idx, meshes)
    ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1], cam.focal_length)
    ref = sc.render_frame(ocam, bluenoise, w, h, frame, depth, flags=O.FLAG_EXT_MATERIALS if ext else 0, threads=8)
    prim = bits(ref["gbuffer_geo"])[..., 3]
    hits = int((prim != 0xFFFFFFFF).sum())
    print("oracle rays", ref["rays"], "camera hits", hits)
    assert ref["rays"][1] > 0.05 * w * h  # the camera sees the scene and paths go on
    if check:
        check(ref, prim, hits)
    r = capi.Renderer(0)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    if ext:
        r.upload_materials(materials)
    r.upload_bluenoise(bluenoise)
    info = r.build_bvh()
    r.set_resolution(w, h)
    r.set_camera(cam)
    r.stats_reset()
    r.render(frame, 1, depth, capi.RENDER_AOV | (capi.RENDER_EXT_MATERIALS if ext else 0))  # AUTO: at most 64 triangles -> fused kernels
    for name, kind in PLANES:
        assert_same(r.readback(kind), ref[name], name)
    s = r.stats()
    assert (s.rays_primary, s.rays_extension, s.rays_shadow) == ref["rays"]
    r.close()
    return info


@pytest.mark.parametrize("seed,nquads,nsingles,fold,ntri", [
    (31, 16, 0, 0.0, 32),   # one mask word, bit 31 in use
    (32, 14, 4, 0.0, 32),   # the same with ids of pairs and loose triangles interleaved
    (33, 16, 1, 0.0, 33),   # smallest two-word scene
    (34, 31, 2, 0.0, 64),   # bit 63 in use
    (35, 15, 2, 0.6, 32),   # folded quads: a ray inside both triangles of a pair
    (36, 30, 3, 0.4, 63),   # ... with two words
])
def test_two_phase_soups(native_lib, bluenoise, seed, nquads, nsingles, fold, ntri):
    scene = fan_soup(seed, nquads, nsingles, fold)
    assert len(scene[3]) // 3 == ntri
    run_case(bluenoise, scene, 96, 80, 5, 3)


@pytest.mark.parametrize("nstack,z0", [(12, -1.0), (28, -4.0)])
def test_two_phase_tunnel(native_lib, bluenoise, nstack, z0):
    """Many candidates per lane, the winner found late, exact ties.  On the CPU the oracle gives rays (2257, 2261, 0), 702 camera
    hits and 351 pixels on the lowest coincident id for the 32-triangle tunnel, (2257, 2449, 0), 756 and 378 for the 64-triangle one."""
    scene = tunnel(nstack, z0)
    assert len(scene[3]) // 3 == 2 * nstack + 8
    lowest = 2 * nstack  # first triangle of the first of the four coincident quads

    def check(ref, prim, hits):
        on_lowest = int((prim == lowest).sum())
        print("pixels on the lowest coincident id", on_lowest)
        assert ref["rays"][1] >= 2 * hits  # paths go on through the stack
        assert on_lowest > 0               # the coincident copies are what the camera sees, and the tie went to the lowest id
        assert int((prim != 0xFFFFFFFF).sum() - (prim == lowest).sum() - (prim == lowest + 1).sum()) == 0

    run_case(bluenoise, scene, 61, 37, 5, 4, check=check)


def test_two_phase_ext(native_lib, bluenoise):
    """The EXT model's bounce >= 1 kernel runs the same loop: 16 planar quads, the last two emissive (next-event rays)."""
    pos, nrm, uv, idx, _ = fan_soup(31, 16, 0, 0.0)
    meshes = np.uint32([[56, 0, 84, 0, 0, 0xFFFFFFFF, 0, 0], [8, 56, 12, 84, 1, 0xFFFFFFFF, 0, 0]])
    idx = idx.copy()
    idx[84:] -= 56
    mats = np.zeros((2, 12), np.float32)
    mats[0, 0:3], mats[0, 3], mats[0, 4:7] = (0.7, 0.6, 0.5), 0.4, (0.04, 0.04, 0.04)
    mats[1, 0:3], mats[1, 3], mats[1, 8:11] = (0.5, 0.5, 0.5), 1.0, (12.0, 11.0, 8.0)

    def check(ref, prim, hits):
        assert ref["rays"][2] > 0  # next-event rays were cast

    run_case(bluenoise, (pos, nrm, uv, idx, meshes), 96, 80, 5, 4, materials=mats, check=check)
