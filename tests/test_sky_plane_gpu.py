"""The sky plane of the small-scene path (small_scene.hip TraceShadeCfg SKYP, k_trace_shade_tab_gray_sky, k_trace_shade_head_gray_sky,
planes.hip k_resolve_coded_sky): a path that escapes at bounce >= 1 stores its throughput -- one float -- into a plane of its own
instead of adding (0.7, 0.7, 0.85) times it to the colour plane with three float atomics, the head launch zeroes that plane for every
(frame slot, padded pixel) of the batch, and the resolve makes the three additions.  Same IEEE operations on the same operands in the
same order, so each case renders with the switch CAP_NO_SKY_PLANE on and off on one context and compares the accumulated sum and every
integer of stats() bit for bit, then the sum and the ray counters with the oracle's; cap_debug_get(CAP_DEBUG_SKY_PLANE) says which form
ran, so that neither passes for the other.  The Cornell box at 70 x 38 (partial tiles in both axes, partial last chunks) and 16 x 8
(two tiles), 1 / 3 / 9 / 64 frame slots, depth 1 (the only escapes are the head's own), 2 (the first later launch) and 8 (the
last-bounce form); a scene open to the sky, a camera that sees nothing, a shard, two accumulating calls, a call cut into batches (the
head re-zeroes a plane that holds the previous batch's throughputs), a reused camera table, the plane's non-zero entries against the
escapes the counters imply, and the renders that must keep the atomics."""
import ctypes as C

import numpy as np
import pytest

import pair_cull_support as S
from capsaicin_amd import capi

pytestmark = pytest.mark.gpu

FIRST = 5
_refs = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def box_camera(w, h):
    cam = capi.cornell_camera(w, h)
    return S.Cam(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.focal_length, cam.sensor_size[0], w, h)


def away_camera(w, h):
    """beside the box, looking along +z, away from it: every camera ray escapes"""
    return S.euler_camera((2.5, 1.0, 6.0), np.pi, 0.0, 0.0, w, h, focal=0.035)


@pytest.fixture(scope="module")
def oracle_scene(cornell_path):
    from oracle import cap_oracle as O
    from oracle import obj_oracle
    g = obj_oracle.load_geometry(cornell_path)
    return O.Scene(g["positions"], g["normals"], g["texcoords"], g["indices"], g["meshes"])


def reference(scene, bluenoise, w, h, cam, first, n, depth):
    """(accumulated sum, rays) by the oracle, once per module run"""
    key = (w, h, cam.__name__, first, n, depth)
    if key not in _refs:
        _refs[key] = scene.render_accumulate(cam(w, h).oracle(), bluenoise, w, h, first, n, depth, threads=8)
    return _refs[key]


def renderer(cornell_path, bluenoise, w, h, cam=box_camera, shard=(0, 1)):
    r = capi.Renderer(0)
    r.upload_geometry(capi.Geometry(cornell_path))
    r.upload_bluenoise(bluenoise)
    info = r.build_bvh()
    assert info.triangle_count <= 64 and r.debug_get(r.DEBUG_SHADE_TAME) == 1  # the kernels that have the form
    r.set_resolution(w, h)
    r.set_shard(*shard)
    r.set_camera(cam(w, h).capi())
    r.debug_switch("CAP_NO_SKY_PLANE", 0)  # (whatever the environment says: these tests are about the plane)
    return r


def owned(w, h, shard):
    tx = (w + 7) // 8
    y, x = np.mgrid[0:h, 0:w]
    return ((y // 8) * tx + x // 8) % shard[1] == shard[0]


def counters(s):
    """every integer of stats(): everything but the timers"""
    return tuple(getattr(s, name) for name, kind in s._fields_ if kind is C.c_uint64)


def rays_of(s):
    return (s.rays_primary, s.rays_extension, s.rays_shadow)


def both_forms(r, calls, depth, form=1):
    """{switch: (sum bits, counters, rays)} of the same calls [(first frame, frames), ..], accumulated, with the atomics (switch 1) and
    with the sky plane (switch 0); `form`: what CAP_DEBUG_SKY_PLANE must say with the switch off"""
    shots = {}
    for off in (1, 0):
        r.debug_switch("CAP_NO_SKY_PLANE", off)
        r.accum_reset()
        r.stats_reset()
        for first, n in calls:
            r.render(first, n, depth, 0)
            assert r.debug_get(r.DEBUG_SKY_PLANE) == (0 if off else form)
        s = r.stats()
        assert s.guard_shade == 0 and s.guard_trace_any == 0 and s.guard_append == 0
        shots[off] = (bits(r.readback(capi.BUF_ACCUM_SUM)).copy(), counters(s), rays_of(s))
    assert shots[0][1] == shots[1][1], "stats() differ between the two forms"
    differ = (shots[0][0] != shots[1][0]).any(-1)
    assert not differ.any(), "the sums of the two forms differ at %d pixels, first (y, x) = %s" % (int(differ.sum()), tuple(np.argwhere(differ)[0]))
    return shots


def assert_oracle(shots, acc, rays, mask=None):
    for off in (1, 0):
        bad = (shots[off][0][..., :3] != bits(acc[..., :3])).any(-1)
        if mask is not None:
            bad &= mask
        assert not bad.any(), "switch %d: the sum differs from the oracle's at %d pixels, first (y, x) = %s" % (off, int(bad.sum()), tuple(np.argwhere(bad)[0]))
        if rays is not None:
            assert shots[off][2] == rays


@pytest.mark.parametrize("depth", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 3, 9, 64])
@pytest.mark.parametrize("size", [(70, 38), (16, 8)], ids=["70x38", "16x8"])
def test_forms_agree_and_match_the_oracle(native_lib, bluenoise, cornell_path, oracle_scene, size, n, depth):
    w, h = size
    acc, rays = reference(oracle_scene, bluenoise, w, h, box_camera, FIRST, n, depth)
    assert rays[1] > 0 and rays[2] > 0
    r = renderer(cornell_path, bluenoise, w, h)
    shots = both_forms(r, [(FIRST, n)], depth)  # one batch: the frames are its slots
    assert r.debug_get(r.DEBUG_GRAY_ENTRIES) == 1 and r.debug_get(r.DEBUG_CAMERA_TABLE) == 1
    r.close()
    assert_oracle(shots, acc, rays)


def test_open_floor(native_lib, bluenoise):
    """tests/test_camera_table_gpu.py's scene under an open sky: most paths escape at bounce 1 or 2, many after a lit first and a lit
    second vertex -- a bounce-0 and a bounce-1 ring entry and, one launch later, the sky store of one path"""
    from oracle import cap_oracle as O
    import test_edge_cases_gpu as T
    w, h, first, n, depth = 64, 40, 3, 9, 2
    arrays, cam = T._open_top_scene(), T._ring_camera(w, h)
    acc, rays = O.Scene(*arrays).render_accumulate(T.ocam(O, cam), bluenoise, w, h, first, n, depth, threads=8)
    r = capi.Renderer(0)
    r.upload_scene(*arrays)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(w, h)
    r.set_camera(cam)
    shots = both_forms(r, [(first, n)], depth)
    escapes = r.debug_get(r.DEBUG_SKY_PLANE_NONZERO)
    print("open floor: extension rays", rays[1], "non-zero sky entries", escapes)
    assert escapes > 0
    r.close()
    assert_oracle(shots, acc, rays)


def test_camera_turned_away(native_lib, bluenoise, cornell_path, oracle_scene):
    """No path has a vertex: the head stores its zeros in waves without a single ray, and nothing else is ever stored"""
    w, h, n, depth = 70, 38, 3, 8
    acc, rays = reference(oracle_scene, bluenoise, w, h, away_camera, FIRST, n, depth)
    assert rays[1] == 0 and rays[2] == 0
    r = renderer(cornell_path, bluenoise, w, h, away_camera)
    # first a render that leaves throughputs in the plane: the zeros below are the second render's own
    r.set_camera(box_camera(w, h).capi())
    r.render(FIRST, n, depth, 0)
    assert r.debug_get(r.DEBUG_SKY_PLANE) == 1 and r.debug_get(r.DEBUG_SKY_PLANE_NONZERO) > 0
    r.set_camera(away_camera(w, h).capi())
    shots = both_forms(r, [(FIRST, n)], depth)
    assert r.debug_get(r.DEBUG_SKY_PLANE_NONZERO) == 0
    r.close()
    assert_oracle(shots, acc, rays)


def test_shard_one_of_three(native_lib, bluenoise, cornell_path, oracle_scene):
    w, h, n, depth = 70, 38, 9, 8
    acc, _ = reference(oracle_scene, bluenoise, w, h, box_camera, FIRST, n, depth)
    r = renderer(cornell_path, bluenoise, w, h, shard=(1, 3))
    shots = both_forms(r, [(FIRST, n)], depth)
    r.close()
    mask = owned(w, h, (1, 3))
    assert mask.any() and not mask.all()
    assert_oracle(shots, acc, None, mask)


def test_two_accumulating_calls(native_lib, bluenoise, cornell_path, oracle_scene):
    """Frames 5 .. 13 in two calls (4 + 5) without a reset: the second call's head zeroes what the first one left"""
    w, h, n, depth = 70, 38, 9, 8
    acc, rays = reference(oracle_scene, bluenoise, w, h, box_camera, FIRST, n, depth)
    r = renderer(cornell_path, bluenoise, w, h)
    shots = both_forms(r, [(FIRST, 4), (FIRST + 4, n - 4)], depth)
    r.close()
    assert_oracle(shots, acc, rays)


def test_one_call_in_batches(native_lib, bluenoise, cornell_path, oracle_scene):
    """Nine frames in batches of 2, 2, 2, 2, 1 slots: every batch's head re-zeroes slots that hold the previous batch's throughputs"""
    w, h, n, depth = 70, 38, 9, 8
    acc, rays = reference(oracle_scene, bluenoise, w, h, box_camera, FIRST, n, depth)
    r = renderer(cornell_path, bluenoise, w, h)
    ppad = ((w + 7) // 8) * ((h + 7) // 8) * 64
    r.set_batch_paths(2 * ppad)
    shots = both_forms(r, [(FIRST, n)], depth)
    assert r.stats().launches_trace_closest == 5 * depth  # five batches
    r.close()
    assert_oracle(shots, acc, rays)


def test_reused_camera_table(native_lib, bluenoise, cornell_path, oracle_scene):
    """The same call twice: the second finds its camera table built, and its head still zeroes the plane"""
    w, h, n, depth = 70, 38, 3, 8
    acc, rays = reference(oracle_scene, bluenoise, w, h, box_camera, FIRST, n, depth)
    r = renderer(cornell_path, bluenoise, w, h)
    r.debug_switch("CAP_NO_TABLE_REUSE", 0)
    for k in range(2):
        r.accum_reset()
        r.stats_reset()
        r.render(FIRST, n, depth, 0)
        assert r.debug_get(r.DEBUG_SKY_PLANE) == 1 and r.debug_get(r.DEBUG_CAMERA_TABLE_REUSED) == k
        assert np.array_equal(bits(r.readback(capi.BUF_ACCUM_SUM)[..., :3]), bits(acc[..., :3]))
        assert rays_of(r.stats()) == rays
    r.close()


def test_nonzero_entries_are_the_escapes(native_lib, bluenoise, cornell_path):
    """Depth 8, 3 slots: every extension ray either finds a vertex or escapes, a vertex of bounce >= 1 is a shaded vertex that a
    depth-0 render of the same frames does not have, and an escaping path's throughput is a product of positive factors."""
    w, h, n, depth = 70, 38, 3, 8
    r = renderer(cornell_path, bluenoise, w, h)
    r.render(FIRST, n, 0, 0)
    assert r.debug_get(r.DEBUG_SKY_PLANE) == 0  # no bounce >= 1 launch
    with pytest.raises(capi.CapError):
        r.debug_get(r.DEBUG_SKY_PLANE_NONZERO)
    first_vertices = r.stats().shaded_vertices
    r.stats_reset()
    r.accum_reset()
    r.render(FIRST, n, depth, 0)
    assert r.debug_get(r.DEBUG_SKY_PLANE) == 1
    s = r.stats()
    escapes = s.rays_extension - (s.shaded_vertices - first_vertices)
    print("extension rays", s.rays_extension, "vertices at bounce >= 1", s.shaded_vertices - first_vertices, "escapes", escapes)
    assert 0 < escapes < s.rays_extension
    assert r.debug_get(r.DEBUG_SKY_PLANE_NONZERO) == escapes
    r.close()


@pytest.mark.parametrize("switch", ["CAP_NO_CAMERA_TABLE", "CAP_NO_GRAY_ENTRIES"])
def test_other_forms_keep_the_atomics(native_lib, bluenoise, cornell_path, oracle_scene, switch):
    w, h, n, depth = 70, 38, 3, 8
    acc, rays = reference(oracle_scene, bluenoise, w, h, box_camera, FIRST, n, depth)
    r = renderer(cornell_path, bluenoise, w, h)
    r.debug_switch(switch, 1)
    shots = both_forms(r, [(FIRST, n)], depth, form=0)
    r.close()
    assert_oracle(shots, acc, rays)


def test_textured_scene_keeps_the_atomics(native_lib, bluenoise):
    """tests/test_gray_entries_gpu.py's four triangles with a texture: three throughput components, no plane"""
    from oracle import cap_oracle as O
    pos = np.float32([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [-3, -1, -1], [3, -1, -1], [3, 2, -1], [-3, 2, -1]])
    nrm = np.tile(np.float32([0, 0, 1]), (8, 1))
    uv = np.float32([[0, 0], [2, 0], [2, 2], [0, 2], [0.1, 0.2], [0.9, 0.2], [0.9, 0.7], [0.1, 0.7]])
    idx = np.uint32([0, 1, 2, 0, 2, 3, 0, 1, 2, 0, 2, 3])
    meshes = np.uint32([[4, 0, 6, 0, 0, 0, 0, 0], [4, 4, 6, 6, 1, 0xFFFFFFFF, 0, 0]])
    tex = np.random.RandomState(5).randint(0, 256, (5, 3, 4)).astype(np.uint8)
    w, h, n, depth = 40, 22, 3, 3
    cam = S.Cam((0.1, 0.3, 4.0), (0, 0, -1), (-1, 0, 0), (0, 1, 0), 0.03, 0.036, w, h)
    acc, rays = O.Scene(pos, nrm, uv, idx, meshes, textures=[tex]).render_accumulate(cam.oracle(), bluenoise, w, h, 9, n, depth, threads=8)
    assert rays[1] > 0
    r = capi.Renderer(0)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    r.upload_texture(0, tex)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(w, h)
    r.set_camera(cam.capi())
    shots = both_forms(r, [(9, n)], depth, form=0)
    r.close()
    assert_oracle(shots, acc, rays)


def test_ext_model_keeps_the_atomics(native_lib, bluenoise):
    """RENDER_EXT_MATERIALS (tests/test_gray_entries_gpu.py's scene): no sample table, no plane, every plane of the frame as the oracle's"""
    from oracle import cap_oracle as O
    import test_pair_carry_gpu as P
    pos, nrm, uv, idx, _ = P.soup(31, "q" * 16, 0.0)
    meshes = np.uint32([[56, 0, 84, 0, 0, 0xFFFFFFFF, 0, 0], [8, 56, 12, 84, 1, 0xFFFFFFFF, 0, 0]])
    idx = idx.copy()
    idx[84:] -= 56
    mats = np.zeros((2, 12), np.float32)
    mats[0, 0:3], mats[0, 3], mats[0, 4:7] = (0.7, 0.6, 0.5), 0.4, (0.04, 0.04, 0.04)
    mats[1, 0:3], mats[1, 3], mats[1, 8:11] = (0.5, 0.5, 0.5), 1.0, (12.0, 11.0, 8.0)
    w, h, depth = 24, 16, 4
    cam = P.camera(w, h)
    ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1], cam.focal_length)
    ref = O.Scene(pos, nrm, uv, idx, meshes, materials=mats).render_frame(ocam, bluenoise, w, h, 5, depth, flags=O.FLAG_EXT_MATERIALS, threads=8)
    r = capi.Renderer(0)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    r.upload_materials(mats)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(w, h)
    r.set_camera(cam)
    r.stats_reset()
    r.render(5, 1, depth, capi.RENDER_AOV | capi.RENDER_EXT_MATERIALS)
    assert r.debug_get(r.DEBUG_SKY_PLANE) == 0
    for name, kind in P.PLANES:
        P.assert_same(r.readback(kind), ref[name], name)
    assert rays_of(r.stats()) == ref["rays"]
    r.close()
