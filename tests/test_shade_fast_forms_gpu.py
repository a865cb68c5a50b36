"""Unscaled square roots and divisions in the shading of the fused small-scene kernels (csrc/cap_unscaled.h, cap_shade.h
map_to_hemisphere_tame, k_trace_shade<..., TAME>): the device self-tests report no differing bit, and renders whose operands sit on
the edges of the proven ranges -- blue-noise texels 0 / 255 and their neighbours (r2 = 0: sin_theta exactly 0; r2 next to 1),
normals with -0 components, unit normals (1, 0, 1e-30) and (0.6, 0.8, 1e-30) that trip the two halves of ortho_vector's guard beside normals that do not, a scene whose
shading records are not tame, a scene that stops being tame and becomes tame again -- equal the oracle's planes bit for bit and its
ray counts, at depth 0 (the bounce-0 kernel alone), 1 and 3 (the skipped sample of the last bounce).  44 x 20 pixels: 6 x 3 tiles of
8 x 8, the last column and row partial; 12 triangles."""
import numpy as np
import pytest

from capsaicin_amd import capi

pytestmark = pytest.mark.gpu

PLANES = (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("direct", capi.BUF_DIRECT), ("indirect", capi.BUF_INDIRECT),
          ("normal_depth", capi.BUF_NORMAL_DEPTH))
W, H = 44, 20
EPS_WALL = (1.0, 0.0, 1e-30)  # unit in fp32; fmaf(a, a, b * b) of ortho_vector's operands (a, b) = (1e-30, 0) underflows to 0
# unit in fp32 too; (a, b) = (1e-30, 0.8): g = 0.64 is inside the guard's first half, a is below 2^-80 and fails its second half, and
# k = 0.8 is no power of two, so a / k and b / k are inexact quotients
SMALL_WALL = (0.6, 0.8, 1e-30)
WALLS = {"axis": (1.0, 0.0, 0.0), "eps": EPS_WALL, "small": SMALL_WALL}


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


def room(left_normal=(1.0, 0.0, 0.0)):
    """An open box seen from +z -- floor, ceiling, back, left and right walls with axis normals, some components -0 -- and a tilted
    quad inside it.  Vertex normals are given per quad (what the shading uses), not derived from the winding."""
    tilt = np.float64([0.3, 0.5, 0.8124])
    tilt /= np.linalg.norm(tilt)
    tu = np.cross(tilt, (0.0, 0.0, 1.0))
    tu /= np.linalg.norm(tu)
    tv = np.cross(tilt, tu)
    quads = [((0, -1, 0), (1.5, 0, 0), (0, 0, 1.2), (-0.0, 1.0, 0.0)),       # floor
             ((0, 1, 0), (1.5, 0, 0), (0, 0, -1.2), (0.0, -1.0, -0.0)),      # ceiling
             ((0, 0, -1.2), (1.5, 0, 0), (0, 1, 0), (0.0, -0.0, 1.0)),       # back wall
             ((-1.5, 0, 0), (0, 0, 1.2), (0, 1, 0), left_normal),            # left wall
             ((1.5, 0, 0), (0, 0, -1.2), (0, 1, 0), (-1.0, 0.0, 0.0)),       # right wall
             ((0.1, -0.3, 0.2), 0.6 * tu, 0.6 * tv, tuple(tilt))]            # tilted quad
    verts, nrm, idx = [], [], []
    for c, u, v, n in quads:
        c, u, v = np.float64(c), np.float64(u), np.float64(v)
        base = len(verts)
        verts += [c - u - v, c + u - v, c + u + v, c - u + v]
        nrm += [n] * 4
        idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    pos = np.float32(verts)
    uv = np.tile(np.float32([[0, 0], [1, 0], [1, 1], [0, 1]]), (len(quads), 1))
    return pos, np.float32(nrm), uv, np.uint32(idx), np.uint32([[len(pos), 0, len(idx), 0, 0, 0xFFFFFFFF, 0, 0]])


def untame_normals(nrm):
    """the floor's first triangle gets opposed vertex normals (vertex 1 of the quad points down)"""
    out = nrm.copy()
    out[1] = (0.0, -1.0, 0.0)
    return out


def camera():
    cam = capi.CameraData()
    cam.position[:] = (0.2, 0.1, 6.0)
    cam.forward[:] = (0, 0, -1)
    cam.right[:] = (-1, 0, 0)
    cam.up[:] = (0, 1, 0)
    cam.focal_length = 0.03
    cam.sensor_size[0] = 0.036
    cam.sensor_size[1] = np.float32(0.036) * (np.float32(H) / np.float32(W))
    return cam


@pytest.fixture(scope="module")
def edge_noise():
    """every texel channel is 0, 1, 254 or 255: samples 0, 1 / 255, 254 / 255 and 1 (whose fraction is 0 again)"""
    rs = np.random.RandomState(7)
    return np.uint8([0, 1, 254, 255])[rs.randint(0, 4, (256, 256, 4))]


_REF = {}


def reference(key, scene, noise, frame, depth):
    """the oracle's frame, computed once per case and shared"""
    k = (key, frame, depth)
    if k not in _REF:
        from oracle import cap_oracle as O
        cam = camera()
        ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1],
                             cam.focal_length)
        _REF[k] = O.Scene(*scene).render_frame(ocam, noise, W, H, frame, depth, threads=8)
    return _REF[k]


def renderer(scene, noise):
    r = capi.Renderer(0)
    r.upload_scene(*scene)
    r.upload_bluenoise(noise)
    r.build_bvh()
    r.set_resolution(W, H)
    r.set_camera(camera())
    return r


def check_frame(r, ref, frame, depth):
    r.stats_reset()
    r.render(frame, 1, depth, capi.RENDER_AOV)  # AUTO: at most 64 triangles -> the fused kernels
    for name, kind in PLANES:
        assert_same(r.readback(kind), ref[name], "%s (frame %d, depth %d)" % (name, frame, depth))
    s = r.stats()
    assert (s.rays_primary, s.rays_extension, s.rays_shadow) == ref["rays"]


def test_selftests(native_lib):
    """every unscaled form against the plain sqrtf or `/` of the same kernel, over every float of its range (unary forms) and over
    more than 2^30 operand pairs inside the guard (ortho_vector's two quotients): no result differs in any bit"""
    r = capi.Renderer(0)
    assert r.debug_get(r.DEBUG_SELFTEST_SHADE_UNARY) == 0
    assert r.debug_get(r.DEBUG_SELFTEST_SHADE_DIV2) == 0
    r.close()


@pytest.mark.parametrize("depth", [0, 1, 3])  # 0: the bounce-0 kernel alone, itself the last bounce
@pytest.mark.parametrize("wall", ["axis", "eps", "small"])
def test_room_edge_noise(native_lib, edge_noise, wall, depth):
    """frames 0 and 1 (sample counters below and above 16: the texel itself, and the texel plus 0.618...) of the room; "eps": and "small":
    the left wall's normal trips ortho_vector's guard, its first and its second half, in every wave that holds one of its vertices"""
    scene = room(WALLS[wall])
    r = renderer(scene, edge_noise)
    assert r.debug_get(r.DEBUG_SHADE_TAME) == 1
    for frame in (0, 1):
        ref = reference(wall, scene, edge_noise, frame, depth)
        if depth:
            assert ref["rays"][1] > 0.2 * W * H  # paths go on
        check_frame(r, ref, frame, depth)
    r.close()


def test_room_bluenoise(native_lib, bluenoise):
    """the product's blue noise, two frames, depth 3"""
    scene = room(EPS_WALL)
    r = renderer(scene, bluenoise)
    for frame in (5, 6):
        check_frame(r, reference("bn", scene, bluenoise, frame, 3), frame, 3)
    r.close()


def test_untame_scene(native_lib, edge_noise):
    """a triangle with opposed vertex normals: the flag reads 0 and the plain forms give the oracle's planes"""
    pos, nrm, uv, idx, meshes = room()
    scene = (pos, untame_normals(nrm), uv, idx, meshes)
    r = renderer(scene, edge_noise)
    assert r.debug_get(r.DEBUG_SHADE_TAME) == 0
    for frame in (0, 1):
        check_frame(r, reference("untame", scene, edge_noise, frame, 3), frame, 3)
    r.close()


def test_untame_and_tame_again(native_lib, edge_noise):
    """cap_scene_update_vertices + refit rewrite the shading records: tame -> untame -> tame, each state rendered"""
    pos, nrm, uv, idx, meshes = room()
    tame, untame = (pos, nrm, uv, idx, meshes), (pos, untame_normals(nrm), uv, idx, meshes)
    r = renderer(tame, edge_noise)
    for key, scene, flag in (("axis", tame, 1), ("untame", untame, 0), ("axis", tame, 1)):
        r.update_vertices(normals=scene[1])
        r.refit_bvh()
        assert r.debug_get(r.DEBUG_SHADE_TAME) == flag
        check_frame(r, reference(key, scene, edge_noise, 1, 3), 1, 3)
    r.close()
