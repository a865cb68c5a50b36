"""32-byte entries of the extension queue (small_scene.hip TraceShadeCfg GRAY, k_trace_shade_tab_gray, k_trace_shade_head_gray): in a
scene without textures the sample-table kernels carry a path's throughput as one float -- its three components are the same operations
on the same operands at every bounce -- and an entry is (origin, throughput) (direction, path id) instead of three float4.  Each case
renders the Cornell box at 70 x 38 -- partial tiles in both axes, and every class's last chunk is partial, so lanes past the end load
the class's last entry from the two arrays that are left -- with the switch CAP_NO_GRAY_ENTRIES on and off on one context and compares
the accumulated sum and every integer of stats() bit for bit, then the sum and the ray counters with the oracle's.
cap_debug_get(CAP_DEBUG_GRAY_ENTRIES) says which form ran, so that neither passes for the other.  Frame slots 1, 3 and 9 (more slots
than the eight jitter groups), depths 1 (the head's entries are never read), 2 and 8, the camera table on (k_trace_shade_head_gray
writes the first entries) and off (the bounce-0 table kernels do), one case on shard 1 of 2.  A textured scene and the EXT model keep
the 48-byte form.  CAP_DEBUG_SELFTEST_GRAY checks the premise itself on the queues a 48-byte render left."""
import ctypes as C

import numpy as np
import pytest

from capsaicin_amd import capi

pytestmark = pytest.mark.gpu

W, H, FIRST = 70, 38, 5
_refs = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def oracle_scene(cornell_path):
    from oracle import cap_oracle as O
    from oracle import obj_oracle
    g = obj_oracle.load_geometry(cornell_path)
    return O.Scene(g["positions"], g["normals"], g["texcoords"], g["indices"], g["meshes"])


def oracle_camera(cam):
    from oracle import cap_oracle as O
    return O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1], cam.focal_length)


def reference(scene, bluenoise, n, depth):
    """(accumulated sum, rays) by the oracle, once per module run"""
    if (n, depth) not in _refs:
        _refs[(n, depth)] = scene.render_accumulate(oracle_camera(capi.cornell_camera(W, H)), bluenoise, W, H, FIRST, n, depth, threads=8)
    return _refs[(n, depth)]


def renderer(cornell_path, bluenoise, shard=(0, 1)):
    r = capi.Renderer(0)
    r.upload_geometry(capi.Geometry(cornell_path))
    r.upload_bluenoise(bluenoise)
    info = r.build_bvh()
    assert info.triangle_count <= 64 and r.debug_get(r.DEBUG_SHADE_TAME) == 1  # the kernels that have the form
    r.set_resolution(W, H)
    r.set_shard(*shard)
    r.set_camera(capi.cornell_camera(W, H))
    return r


def owned(shard):
    tx = (W + 7) // 8
    y, x = np.mgrid[0:H, 0:W]
    return ((y // 8) * tx + x // 8) % shard[1] == shard[0]


def counters(s):
    """every integer of stats(): everything but the timers"""
    return tuple(getattr(s, name) for name, kind in s._fields_ if kind is C.c_uint64)


def both_forms(r, n, depth, camera_table):
    """{switch: (sum bits, counters, rays)} of the same render in the 48-byte form (1) and the 32-byte form (0)"""
    r.debug_switch("CAP_NO_CAMERA_TABLE", 0 if camera_table else 1)
    shots = {}
    for off in (1, 0):
        r.debug_switch("CAP_NO_GRAY_ENTRIES", off)
        r.accum_reset()
        r.stats_reset()
        r.render(FIRST, n, depth, 0)  # one batch: the frames are its slots
        assert r.debug_get(r.DEBUG_GRAY_ENTRIES) == 1 - off
        assert r.debug_get(r.DEBUG_SAMPLE_TABLE) == 1
        assert r.debug_get(r.DEBUG_CAMERA_TABLE) == (1 if camera_table else 0)
        s = r.stats()
        assert s.guard_shade == 0 and s.guard_trace_any == 0 and s.guard_append == 0
        shots[off] = (bits(r.readback(capi.BUF_ACCUM_SUM)).copy(), counters(s), (s.rays_primary, s.rays_extension, s.rays_shadow))
    assert shots[0][1] == shots[1][1], "stats() differ between the entry forms"
    differ = (shots[0][0] != shots[1][0]).any(-1)
    assert not differ.any(), "the sums of the two entry forms differ at %d pixels, first (y, x) = %s" % (int(differ.sum()), tuple(np.argwhere(differ)[0]))
    return shots


@pytest.mark.parametrize("camera_table", [True, False], ids=["camera table", "bounce 0 launched"])
@pytest.mark.parametrize("depth", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 3, 9])
def test_forms_agree_and_match_the_oracle(native_lib, bluenoise, cornell_path, oracle_scene, n, depth, camera_table):
    acc, rays = reference(oracle_scene, bluenoise, n, depth)
    assert rays[1] > 0 and rays[2] > 0
    r = renderer(cornell_path, bluenoise)
    shots = both_forms(r, n, depth, camera_table)
    r.close()
    for off in (1, 0):
        bad = (shots[off][0][..., :3] != bits(acc[..., :3])).any(-1)
        assert not bad.any(), "switch %d: the sum differs from the oracle's at %d pixels, first (y, x) = %s" % (off, int(bad.sum()), tuple(np.argwhere(bad)[0]))
        assert shots[off][2] == rays


def test_shard_one_of_two(native_lib, bluenoise, cornell_path, oracle_scene):
    """the shard's own pixels of the sum; the two shards' rays add up to the oracle's"""
    n, depth = 9, 8
    acc, rays = reference(oracle_scene, bluenoise, n, depth)
    total = np.zeros(3, np.int64)
    for shard in ((1, 2), (0, 2)):
        r = renderer(cornell_path, bluenoise, shard)
        shots = both_forms(r, n, depth, True)
        r.close()
        mask = owned(shard)
        assert mask.any()
        bad = (shots[0][0][..., :3] != bits(acc[..., :3])).any(-1) & mask
        assert not bad.any(), "shard %d: the sum differs from the oracle's at %d pixels" % (shard[0], int(bad.sum()))
        total += shots[0][2]
    assert tuple(int(x) for x in total) == rays


def test_textured_scene_keeps_48_bytes(native_lib, bluenoise):
    """Four triangles, one texture on the front quad: kd differs between the components, the table kernels run with 48-byte entries"""
    from oracle import cap_oracle as O
    pos = np.float32([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [-3, -1, -1], [3, -1, -1], [3, 2, -1], [-3, 2, -1]])
    nrm = np.tile(np.float32([0, 0, 1]), (8, 1))
    uv = np.float32([[0, 0], [2, 0], [2, 2], [0, 2], [0.1, 0.2], [0.9, 0.2], [0.9, 0.7], [0.1, 0.7]])
    idx = np.uint32([0, 1, 2, 0, 2, 3, 0, 1, 2, 0, 2, 3])
    meshes = np.uint32([[4, 0, 6, 0, 0, 0, 0, 0], [4, 4, 6, 6, 1, 0xFFFFFFFF, 0, 0]])
    tex = np.random.RandomState(5).randint(0, 256, (5, 3, 4)).astype(np.uint8)
    w, h, n, depth = 40, 22, 3, 3
    cam = capi.CameraData()
    cam.position[:] = (0.1, 0.3, 4.0)
    cam.forward[:] = (0, 0, -1)
    cam.right[:] = (-1, 0, 0)
    cam.up[:] = (0, 1, 0)
    cam.focal_length = 0.03
    cam.sensor_size[0] = 0.036
    cam.sensor_size[1] = np.float32(0.036) * (np.float32(h) / np.float32(w))
    acc, rays = O.Scene(pos, nrm, uv, idx, meshes, textures=[tex]).render_accumulate(oracle_camera(cam), bluenoise, w, h, 9, n, depth, threads=8)
    assert rays[1] > 0
    r = capi.Renderer(0)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    r.upload_texture(0, tex)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(w, h)
    r.set_camera(cam)
    r.render(9, n, depth, 0)
    assert r.debug_get(r.DEBUG_SAMPLE_TABLE) == 1 and r.debug_get(r.DEBUG_GRAY_ENTRIES) == 0
    assert np.array_equal(bits(r.readback(capi.BUF_ACCUM_SUM)[..., :3]), bits(acc[..., :3]))
    s = r.stats()
    assert (s.rays_primary, s.rays_extension, s.rays_shadow) == rays
    v = r.debug_get(r.DEBUG_SELFTEST_GRAY)  # the negative control of the self-test: here the components do differ
    print("textured: entries", v & 0xffffffff, "with unequal components", v >> 32)
    assert v >> 32 > 0
    r.close()


def test_ext_model_keeps_48_bytes(native_lib, bluenoise):
    """RENDER_EXT_MATERIALS: no sample table, three throughput components, every plane as the oracle's"""
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
    ref = O.Scene(pos, nrm, uv, idx, meshes, materials=mats).render_frame(oracle_camera(cam), bluenoise, w, h, 5, depth, flags=O.FLAG_EXT_MATERIALS, threads=8)
    r = capi.Renderer(0)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    r.upload_materials(mats)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(w, h)
    r.set_camera(cam)
    r.stats_reset()
    r.render(5, 1, depth, capi.RENDER_AOV | capi.RENDER_EXT_MATERIALS)
    assert r.debug_get(r.DEBUG_GRAY_ENTRIES) == 0 and r.debug_get(r.DEBUG_SAMPLE_TABLE) == 0
    for name, kind in P.PLANES:
        P.assert_same(r.readback(kind), ref[name], name)
    s = r.stats()
    assert (s.rays_primary, s.rays_extension, s.rays_shadow) == ref["rays"]
    with pytest.raises(capi.CapError):
        r.debug_get(r.DEBUG_SELFTEST_GRAY)  # the premise is the reference model's
    r.close()


@pytest.mark.parametrize("camera_table", [True, False], ids=["camera table", "bounce 0 launched"])
def test_the_premise_on_the_device(native_lib, bluenoise, cornell_path, camera_table):
    """After a 48-byte render of 3 slots at depth 8: every entry the last two appending bounces left, up to the class counts, has three
    bitwise equal throughput words.  After a 32-byte render there is nothing to look at and the getter refuses."""
    r = renderer(cornell_path, bluenoise)
    r.debug_switch("CAP_NO_CAMERA_TABLE", 0 if camera_table else 1)
    r.debug_switch("CAP_NO_GRAY_ENTRIES", 1)
    r.render(FIRST, 3, 8, 0)
    assert r.debug_get(r.DEBUG_GRAY_ENTRIES) == 0
    v = r.debug_get(r.DEBUG_SELFTEST_GRAY)
    print("entries looked at", v & 0xffffffff, "with unequal components", v >> 32)
    assert v & 0xffffffff > 0
    assert v >> 32 == 0
    r.debug_switch("CAP_NO_GRAY_ENTRIES", None)
    r.render(FIRST, 3, 8, 0)
    assert r.debug_get(r.DEBUG_GRAY_ENTRIES) == 1
    with pytest.raises(capi.CapError):
        r.debug_get(r.DEBUG_SELFTEST_GRAY)
    r.close()
