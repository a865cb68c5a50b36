"""Reuse of the camera-vertex table (ctx_render.hip CameraTableKey, CAP_DEBUG_CAMERA_TABLE_REUSED): a batch launches no builder when
its working set's table was built from the same camera, screen and shard, group jitters and scene records.  A reused table must be the
table a build would give -- CAP_DEBUG_SELFTEST_CAMERA_TABLE re-evaluates every entry on the device and finds 0 differing -- and the
key must miss after everything the builder reads has changed: camera, resolution, shard, vertices (update + refit), materials, the
jitter groups (another first frame, another group count).  After each change the next call reports a rebuild, the self-test finds 0
differing entries and the sum is the oracle's.  Cornell box, 70 x 38, depth 2, every comparison exact."""
import numpy as np
import pytest

import pair_cull_support as S
import test_camera_table_gpu as T
from capsaicin_amd import capi

pytestmark = pytest.mark.gpu

W, H, DEPTH = 70, 38, 2


def moved_camera(w, h):
    """the Cornell view from a little to the side and closer"""
    cam = capi.cornell_camera(w, h)
    position = np.float32(tuple(cam.position)) + np.float32([0.06, 0.03, -0.12])
    return S.Cam(tuple(position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.focal_length, cam.sensor_size[0], w, h)


@pytest.fixture(scope="module")
def geometry(cornell_path):
    from oracle import obj_oracle
    return obj_oracle.load_geometry(cornell_path)


def oracle_of(geometry, positions=None):
    from oracle import cap_oracle as O
    g = geometry
    return O.Scene(g["positions"] if positions is None else positions, g["normals"], g["texcoords"], g["indices"], g["meshes"])


def renderer(geometry, bluenoise, w=W, h=H, cam=T.box_camera):
    g = geometry
    r = capi.Renderer(0)
    r.upload_scene(g["positions"], g["normals"], g["texcoords"], g["indices"], g["meshes"])
    r.upload_bluenoise(bluenoise)
    info = r.build_bvh()
    assert info.triangle_count <= 64 and r.debug_get(r.DEBUG_SHADE_TAME) == 1
    r.set_resolution(w, h)
    r.set_camera(cam(w, h).capi())
    r.debug_switch("CAP_NO_TABLE_REUSE", 0)  # (whatever the environment says: these tests are about the reuse)
    return r


def shot(r, first, n, reused, slots=None, groups=None):
    """one call into a fresh accumulation: the getter, the table against its definition; returns (sum bits, counters)"""
    r.accum_reset()
    r.stats_reset()
    r.render(first, n, DEPTH, 0)
    assert r.debug_get(r.DEBUG_CAMERA_TABLE) == 1
    assert r.debug_get(r.DEBUG_CAMERA_TABLE_REUSED) == (1 if reused else 0)
    v = r.debug_get(r.DEBUG_SELFTEST_CAMERA_TABLE)
    assert v >> 32 == 0, "%d entries of the %s table differ from bounce 0's camera vertices" % (v >> 32, "reused" if reused else "built")
    assert v & 0xffff == (n if slots is None else slots)
    if groups is not None:
        assert (v >> 16) & 0xffff == groups
    s = r.stats()
    T.assert_clean(s)
    return T.bits(r.readback(capi.BUF_ACCUM_SUM)).copy(), T.counters(s), T.rays_of(s)


def assert_oracle(got, scene, bluenoise, w, h, cam, first, n, mask=None):
    acc, rays = scene.render_accumulate(cam(w, h).oracle(), bluenoise, w, h, first, n, DEPTH, threads=8)
    bad = (got[0][..., :3] != T.bits(acc[..., :3])).any(-1)
    if mask is not None:
        bad &= mask
    else:
        assert got[2] == rays
    assert not bad.any(), "the sum differs from the oracle's at %d pixels, first (y, x) = %s" % (int(bad.sum()), tuple(np.argwhere(bad)[0]))


def test_two_equal_calls(native_lib, bluenoise, geometry):
    scene = oracle_of(geometry)
    r = renderer(geometry, bluenoise)
    a = shot(r, 0, 16, False, groups=8)
    b = shot(r, 0, 16, True, groups=8)
    r.debug_switch("CAP_NO_TABLE_REUSE", 1)
    c = shot(r, 0, 16, False)
    r.debug_switch("CAP_NO_TABLE_REUSE", 0)
    d = shot(r, 0, 16, True)  # the table the switched-off render built is a table like any other
    for x in (b, c, d):
        assert x[1] == a[1] and np.array_equal(x[0], a[0])
    assert_oracle(a, scene, bluenoise, W, H, T.box_camera, 0, 16)
    r.close()


def test_every_input_of_the_builder_misses_the_key(native_lib, bluenoise, geometry):
    scene = oracle_of(geometry)
    r = renderer(geometry, bluenoise)
    first, n = 0, 5
    shot(r, first, n, False)
    assert_oracle(shot(r, first, n, True), scene, bluenoise, W, H, T.box_camera, first, n)
    # a moved camera
    r.set_camera(moved_camera(W, H).capi())
    assert_oracle(shot(r, first, n, False), scene, bluenoise, W, H, moved_camera, first, n)
    shot(r, first, n, True)
    # another resolution
    w2, h2 = 72, 40
    r.set_resolution(w2, h2)
    r.set_camera(moved_camera(w2, h2).capi())
    assert_oracle(shot(r, first, n, False), scene, bluenoise, w2, h2, moved_camera, first, n)
    shot(r, first, n, True)
    r.set_resolution(W, H)
    r.set_camera(T.box_camera(W, H).capi())
    shot(r, first, n, False)
    # another shard
    r.set_shard(1, 3)
    assert_oracle(shot(r, first, n, False), scene, bluenoise, W, H, T.box_camera, first, n, mask=T.owned(W, H, (1, 3)))
    shot(r, first, n, True)
    r.set_shard(0, 1)
    shot(r, first, n, False)
    # vertices moved inside the view: one of the two boxes lifted and pushed
    g = geometry
    moved = np.array(g["positions"], np.float32).reshape(-1, 3).copy()
    meshes = np.asarray(g["meshes"], np.uint32).reshape(-1, 8)  # rows (vertex count, first vertex, index count, first index, ...)
    counts = [int(d[2]) for d in meshes]
    m = meshes[int(np.argmax(counts))]
    moved[int(m[1]):int(m[1]) + int(m[0])] += np.float32([0.11, 0.07, 0.05])
    before = shot(r, first, n, True)
    r.update_vertices(positions=moved)
    r.refit_bvh()
    after = shot(r, first, n, False)
    assert not np.array_equal(before[0], after[0])  # the moved vertices are in the view
    assert_oracle(after, oracle_of(geometry, moved), bluenoise, W, H, T.box_camera, first, n)
    shot(r, first, n, True)
    r.update_vertices(positions=np.array(g["positions"], np.float32))
    r.refit_bvh()
    assert_oracle(shot(r, first, n, False), scene, bluenoise, W, H, T.box_camera, first, n)
    # a material upload (the reference model's first-vertex code comes from the scene's diffuse constant)
    mats = np.zeros((len(counts), 12), np.float32)
    mats[:, 0:3] = 0.5
    mats[:, 3] = 1.0
    r.upload_materials(mats)
    assert_oracle(shot(r, first, n, False), scene, bluenoise, W, H, T.box_camera, first, n)
    shot(r, first, n, True)
    # other jitter groups: 5 frames from 3 instead of from 0
    assert_oracle(shot(r, 3, n, False), scene, bluenoise, W, H, T.box_camera, 3, n)
    shot(r, 3, n, True)
    # another frame count: six groups instead of five
    assert_oracle(shot(r, 3, 6, False), scene, bluenoise, W, H, T.box_camera, 3, 6)
    r.close()


def test_the_next_64_frames_reuse(native_lib, bluenoise, geometry):
    """any 64 consecutive frames hold the same eight jitters in the same order of first appearance: frames 64 .. 127 read the table of 0 .. 63"""
    scene = oracle_of(geometry)
    r = renderer(geometry, bluenoise)
    shot(r, 0, 64, False, groups=8)
    assert_oracle(shot(r, 64, 64, True, groups=8), scene, bluenoise, W, H, T.box_camera, 64, 64)
    # ... and 16 frames from 8 have the groups of 64 from 0: the key holds the groups' jitters, not the frames
    shot(r, 8, 16, True, groups=8)
    r.close()


def test_second_batch_of_a_call_reuses(native_lib, bluenoise, geometry):
    scene = oracle_of(geometry)
    r = renderer(geometry, bluenoise)
    ppad = ((W + 7) // 8) * ((H + 7) // 8) * 64
    r.set_batch_paths(8 * ppad)  # 16 frames: two batches of eight slots, the same eight jitters in the same order
    got = shot(r, 0, 16, True, slots=8, groups=8)  # (a fresh context: the first batch built, or the self-test would not find its table)
    assert r.stats().frames == 16
    assert_oracle(got, scene, bluenoise, W, H, T.box_camera, 0, 16)
    r.debug_switch("CAP_NO_TABLE_REUSE", 1)
    off = shot(r, 0, 16, False, slots=8, groups=8)
    assert off[1] == got[1] and np.array_equal(off[0], got[0])
    r.close()


def test_a_refused_call_drops_the_key(native_lib, bluenoise, geometry):
    r = renderer(geometry, bluenoise)
    a = shot(r, 0, 5, False)
    shot(r, 0, 5, True)
    with pytest.raises(capi.CapError):
        r.render(0, 5, 256, 0)  # num_bounces beyond 255: refused before anything is launched
    b = shot(r, 0, 5, False)
    assert b[1] == a[1] and np.array_equal(b[0], a[0])
    shot(r, 0, 5, True)
    r.close()
