"""Bounce 0 inside bounce 1's launch, from a table of camera vertices (small_scene.hip k_camera_vertices, k_trace_shade_head): the frame
slots of a batch share eight sub-pixel jitters, so the camera rays are traced once per (jitter group, pixel) into a table, and the
per-slot remainder of bounce 0 -- light term, probe, sampled direction, throughput -- runs at the head of every chunk of the batch's
first bounce >= 1 launch, which keeps the ray in registers; bounce 0's shadow rays go through the wave rings.  The form exists in
accumulate-only renders (no CAP_RENDER_AOV), so what is compared is the accumulated sum, bit for bit against the oracle's sum in frame
order, every ray counter and the guards; with CAP_RENDER_AOV or at depth 0 the getter must say that bounce 0 was its own launch, and
then every plane is compared as well.  cap_debug_get(CAP_DEBUG_CAMERA_TABLE) says which form ran, so that neither passes for the other.
The shapes are the smallest at which the grouping and the indices can go wrong: all eight groups with eight slots each, groups of two
and one that are not contiguous, a wrap of frame_count mod 8 inside a batch, partial tiles, three shards, the fused launch as the last
bounce, tiles without a vertex, and a scene open to the light where one path has a bounce-0 and a bounce-1 entry in one wave's ring."""
import ctypes as C

import numpy as np
import pytest

import pair_cull_support as S
from capsaicin_amd import capi

pytestmark = pytest.mark.gpu

PLANES = (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("direct", capi.BUF_DIRECT), ("albedo", capi.BUF_ALBEDO),
          ("normal_depth", capi.BUF_NORMAL_DEPTH), ("indirect", capi.BUF_INDIRECT), ("combined", capi.BUF_COMBINED))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def box_camera(w, h):
    cam = capi.cornell_camera(w, h)
    return S.Cam(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.focal_length, cam.sensor_size[0], w, h)


def turned_camera(w, h):
    """from outside and to the side of the box: whole tiles of sky, tiles the box's silhouette cuts, tiles inside it"""
    return S.euler_camera((2.5, 1.0, 6.0), 0.5, -0.05, 0.1, w, h, focal=0.035)


# name: (width, height, camera, first frame, frames, depth)
CASES = {
    "eight groups of eight": (16, 8, box_camera, 0, 64, 4),
    "groups of two and one": (100, 52, box_camera, 5, 9, 4),       # frames 5 .. 13: jitters 5 6 7 0 1 2 3 4 5 -- slots 0 and 8 share one
    "partial tiles, wrap of mod 8": (104, 56, box_camera, 1021, 24, 4),  # 1021 mod 8 = 5: every group's slots are 8 apart, starting mid-cycle
    "last bounce": (100, 52, box_camera, 5, 9, 1),                 # depth 1: the fused launch samples nothing for bounce 1 and emits nothing
    "tiles with no vertex": (100, 52, turned_camera, 3, 16, 4),
    "three shards": (104, 56, box_camera, 5, 16, 4),
}
_refs = {}


@pytest.fixture(scope="module")
def oracle_scene(cornell_path):
    from oracle import cap_oracle as O
    from oracle import obj_oracle
    g = obj_oracle.load_geometry(cornell_path)
    return O.Scene(g["positions"], g["normals"], g["texcoords"], g["indices"], g["meshes"])


def reference(scene, bluenoise, w, h, cam, first, n, depth):
    """(accumulated sum, rays) by the oracle, once per module run"""
    key = (id(scene), w, h, cam.__name__, first, n, depth)
    if key not in _refs:
        _refs[key] = scene.render_accumulate(cam(w, h).oracle(), bluenoise, w, h, first, n, depth, threads=8)
    return _refs[key]


def renderer(cornell_path, bluenoise, w, h, cam, shard=(0, 1)):
    r = capi.Renderer(0)
    r.upload_geometry(capi.Geometry(cornell_path))
    r.upload_bluenoise(bluenoise)
    info = r.build_bvh()
    assert info.triangle_count <= 64 and r.debug_get(r.DEBUG_SHADE_TAME) == 1  # the kernels that have the form
    r.set_resolution(w, h)
    r.set_shard(*shard)
    r.set_camera(cam(w, h).capi())
    return r


def owned(w, h, shard):
    tx = (w + 7) // 8
    y, x = np.mgrid[0:h, 0:w]
    return ((y // 8) * tx + x // 8) % shard[1] == shard[0]


def assert_sum(r, acc, mask=None):
    bad = (bits(r.readback(capi.BUF_ACCUM_SUM)[..., :3]) != bits(acc[..., :3])).any(-1)
    if mask is not None:
        bad &= mask
    assert not bad.any(), "the sum differs at %d pixels, first (y, x) = %s" % (int(bad.sum()), tuple(np.argwhere(bad)[0]))


def assert_clean(s):
    assert s.guard_shade == 0 and s.guard_trace_any == 0 and s.guard_append == 0


def rays_of(s):
    return (s.rays_primary, s.rays_extension, s.rays_shadow)


def counters(s):
    """every integer of stats(): everything but the timers"""
    return tuple(getattr(s, name) for name, kind in s._fields_ if kind is C.c_uint64)


@pytest.mark.parametrize("name", [n for n in CASES if n != "three shards"])
def test_oracle_parity(native_lib, bluenoise, cornell_path, oracle_scene, name):
    w, h, cam, first, n, depth = CASES[name]
    acc, rays = reference(oracle_scene, bluenoise, w, h, cam, first, n, depth)
    assert rays[1] > 0 and rays[2] > 0
    if name == "tiles with no vertex":
        ref = oracle_scene.render_frame(cam(w, h).oracle(), bluenoise, w, h, first, depth, threads=8)
        sky = bits(ref["gbuffer_geo"])[..., 3] == capi.MISS
        assert any(sky[y:y + 8, x:x + 8].all() for y in range(0, h - 7, 8) for x in range(0, w - 7, 8))  # a whole tile of sky
    r = renderer(cornell_path, bluenoise, w, h, cam)
    r.render(first, n, depth, 0)  # one batch: the frames are its slots
    assert r.debug_get(r.DEBUG_CAMERA_TABLE) == 1
    assert_sum(r, acc)
    s = r.stats()
    assert rays_of(s) == rays
    assert s.launches_trace_any == 1 and s.launches_trace_closest == depth  # as with bounce 0 as a launch: every field of stats() keeps its value
    assert s.rays_extension_bounce0 > 0 and s.rays_shadow_bounce0 > s.shadow_entries_bounce0 > 0  # bounce 0's own counter words
    assert_clean(s)
    r.close()


def test_three_shards(native_lib, bluenoise, cornell_path, oracle_scene):
    """16 frames at 104 x 56 (13 x 7 tiles) over three shards: every shard's own pixels of the sum, and the shards' rays add up."""
    w, h, cam, first, n, depth = CASES["three shards"]
    acc, rays = reference(oracle_scene, bluenoise, w, h, cam, first, n, depth)
    total = np.zeros(3, np.int64)
    for index in (1, 0, 2):
        r = renderer(cornell_path, bluenoise, w, h, cam, (index, 3))
        r.render(first, n, depth, 0)
        assert r.debug_get(r.DEBUG_CAMERA_TABLE) == 1
        mask = owned(w, h, (index, 3))
        assert mask.any()
        assert_sum(r, acc, mask)
        s = r.stats()
        assert_clean(s)
        total += rays_of(s)
        r.close()
    assert tuple(int(x) for x in total) == rays


def test_forms_without_the_table(native_lib, bluenoise, cornell_path, oracle_scene):
    """Depth 0 has no bounce >= 1 launch and CAP_RENDER_AOV needs bounce 0's planes: the getter says bounce 0 ran as its own launch, the
    self-test refuses, and the results are the oracle's -- every plane of the last frame included."""
    w, h, first, n = 100, 52, 5, 9
    r = renderer(cornell_path, bluenoise, w, h, box_camera)
    acc0, rays0 = reference(oracle_scene, bluenoise, w, h, box_camera, first, n, 0)
    r.render(first, n, 0, 0)
    assert r.debug_get(r.DEBUG_CAMERA_TABLE) == 0
    with pytest.raises(capi.CapError):
        r.debug_get(r.DEBUG_SELFTEST_CAMERA_TABLE)
    assert_sum(r, acc0)
    assert rays_of(r.stats()) == rays0
    r.accum_reset()
    r.stats_reset()
    acc, rays = reference(oracle_scene, bluenoise, w, h, box_camera, first, n, 4)
    last = oracle_scene.render_frame(box_camera(w, h).oracle(), bluenoise, w, h, first + n - 1, 4, threads=8)
    r.render(first, n, 4, capi.RENDER_AOV)
    assert r.debug_get(r.DEBUG_CAMERA_TABLE) == 0
    for name, kind in PLANES:
        bad = (bits(r.readback(kind)) != bits(last[name])).any(-1)
        assert not bad.any(), "%s: %d pixels differ" % (name, int(bad.sum()))
    assert_sum(r, acc)
    s = r.stats()
    assert rays_of(s) == rays and s.launches_trace_any == 1
    assert_clean(s)
    r.close()


def test_open_floor_both_vertices_lit(native_lib, bluenoise):
    """A floor, two low walls and a panel under an open sky: most shadow rays are unoccluded, so a path parks a bounce-0 and a bounce-1
    entry in its wave's ring within one chunk, and both are often traced together -- the first stores color.w alone, the second adds
    to color.xyz.  The oracle's planes of one frame at depth 1 say that such paths exist: the first vertex lit (direct != 0) and the
    second one lit as well -- indirect.x != indirect.y, which the light's colour gives and the grey sky term (0.7, 0.7, 0.85) cannot."""
    from oracle import cap_oracle as O
    import test_edge_cases_gpu as T
    w, h, first, n, depth = 64, 40, 3, 9, 2
    arrays, cam = T._open_top_scene(), T._ring_camera(w, h)
    scene = O.Scene(*arrays)
    one = scene.render_frame(T.ocam(O, cam), bluenoise, w, h, first, 1, threads=8)
    both = (one["direct"][..., :3] != 0).any(-1) & (one["indirect"][..., 0] != one["indirect"][..., 1])
    print("paths lit at both vertices:", int(both.sum()), "of", w * h)
    assert both.sum() >= 64  # more than one chunk of them
    acc, rays = scene.render_accumulate(T.ocam(O, cam), bluenoise, w, h, first, n, depth, threads=8)
    r = capi.Renderer(0)
    r.upload_scene(*arrays)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(w, h)
    r.set_camera(cam)
    r.render(first, n, depth, 0)
    assert r.debug_get(r.DEBUG_CAMERA_TABLE) == 1
    got = r.readback(capi.BUF_ACCUM_SUM)
    assert np.array_equal(bits(got[..., :3]), bits(acc[..., :3])) and np.all(got[..., 3] == n)
    s = r.stats()
    assert rays_of(s) == rays
    assert s.shadow_entries_bounce0 > 0.8 * s.rays_shadow_bounce0  # the probe answers little here: bounce 0's rays are ring entries
    assert_clean(s)
    r.close()


def test_two_accumulating_calls(native_lib, bluenoise, cornell_path, oracle_scene):
    """Frames 5 .. 13 in two calls (4 + 5: other groups, another table) without a reset: the sum of all nine in frame order."""
    w, h, cam, first, n, depth = CASES["groups of two and one"]
    acc, rays = reference(oracle_scene, bluenoise, w, h, cam, first, n, depth)
    r = renderer(cornell_path, bluenoise, w, h, cam)
    r.render(first, 4, depth, 0)
    assert r.debug_get(r.DEBUG_CAMERA_TABLE) == 1
    r.render(first + 4, n - 4, depth, 0)
    assert r.debug_get(r.DEBUG_CAMERA_TABLE) == 1
    assert_sum(r, acc)
    s = r.stats()
    assert rays_of(s) == rays
    assert_clean(s)
    r.close()


def test_switch_parity_in_one_process(native_lib, bluenoise, cornell_path):
    """The same renders on one context with CAP_NO_CAMERA_TABLE on and off: the accumulated sum and every counter of stats() equal as bits."""
    w, h = 100, 52
    r = renderer(cornell_path, bluenoise, w, h, box_camera)
    shots = {}
    for off in (1, 0, 1, 0):
        r.debug_switch("CAP_NO_CAMERA_TABLE", off)
        got = []
        for first, n, depth in ((5, 9, 4), (1021, 24, 8), (7, 2, 1), (0, 64, 2)):
            r.accum_reset()
            r.stats_reset()
            r.render(first, n, depth, 0)
            assert r.debug_get(r.DEBUG_CAMERA_TABLE) == 1 - off
            s = r.stats()
            assert_clean(s)
            got.append((bits(r.readback(capi.BUF_ACCUM_SUM)).copy(), counters(s)))
        shots.setdefault(off, []).append(got)
    for a, b in ((shots[1][0], shots[0][0]), (shots[1][1], shots[0][1]), (shots[0][0], shots[0][1])):
        for (sa, ca), (sb, cb) in zip(a, b):
            assert ca == cb
            assert np.array_equal(sa, sb)
    r.close()


def test_the_table_itself(native_lib, bluenoise, cornell_path):
    """Every entry of the table a render left: bounce 0's camera vertex of every (slot, padded pixel), evaluated on the device with the
    slot's own frame constants, against the entry of the slot's group -- position, code, normal and the spare word, no bit may differ.
    Nine frames from 5 at 100 x 52: eight groups, one of two slots that are eight apart, partial tiles and padding lanes."""
    r = renderer(cornell_path, bluenoise, 100, 52, box_camera)
    r.render(5, 9, 2, 0)
    assert r.debug_get(r.DEBUG_CAMERA_TABLE) == 1
    v = r.debug_get(r.DEBUG_SELFTEST_CAMERA_TABLE)
    print("slots", v & 0xffff, "groups", (v >> 16) & 0xffff, "mismatches", v >> 32)
    assert v & 0xffff == 9 and (v >> 16) & 0xffff == 8
    assert v >> 32 == 0
    r.render(0, 64, 1, 0)
    v = r.debug_get(r.DEBUG_SELFTEST_CAMERA_TABLE)
    assert v & 0xffff == 64 and (v >> 16) & 0xffff == 8 and v >> 32 == 0
    r.close()
