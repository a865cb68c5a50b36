"""Direction-sample terms from a per-batch table (small_scene.hip k_sample_terms, the TAB kernels of k_trace_shade_tab): what shading
makes of a vertex's blue-noise sample before it looks at the hit -- sincos of the azimuth, the two square roots -- is evaluated once per
(sampling bounce, frame slot, position in the 64 x 64 blue-noise period) and the fused small-scene kernels load the three terms.  Cornell
box, reference model.  Every plane, the accumulated sum and every ray counter bit for bit against the oracle with the table, and against
the same context with the table switched off (CAP_SAMPLE_TABLE = 0: the kernels that carry the sample in the queue entries);
cap_debug_get(CAP_DEBUG_SAMPLE_TABLE) says which form ran, so that neither can pass for the other.  The shapes are the smallest at which
the index can go wrong: both axes past the 64-pixel period, tiles_x = 13, partial tiles, two chunks, frame slots with every 4 x 4 texel
offset, large count / 16, depth 1 (only bounce 0 samples), three shards."""
import ctypes as C

import numpy as np
import pytest

from capsaicin_amd import capi

pytestmark = pytest.mark.gpu

PLANES = (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("direct", capi.BUF_DIRECT), ("albedo", capi.BUF_ALBEDO),
          ("normal_depth", capi.BUF_NORMAL_DEPTH), ("indirect", capi.BUF_INDIRECT), ("combined", capi.BUF_COMBINED))

# (width, height, first frame, frames, depth)
CASES = [
    (136, 72, 3, 1, 4),     # 17 x 9 tiles: both axes past the 64-pixel period
    (104, 56, 3, 1, 4),     # tiles_x = 13
    (100, 52, 3, 1, 4),     # partial tiles on the right and bottom edges
    (16, 8, 3, 1, 4),       # two chunks
    (104, 56, 5, 9, 4),     # nine slots
    (100, 52, 5, 2, 8),     # frames 5 and 6 at depth 8: count mod 16 = 13 .. 5 and 6 .. 14 over bounces 0 .. 8, every 4 x 4 offset between them
    (16, 8, 1021, 24, 4),   # count / 16 = 1595 .. 1631: k near 1 000, t + k keeps 14 fraction bits
    (104, 56, 4095, 2, 4),  # count / 16 = 6398 .. 6400: k near 4 000, 12 fraction bits
    (136, 72, 3, 1, 1),     # depth 1: only bounce 0 samples
    (16, 8, 3, 1, 8),       # depth 8 in two chunks: classes that run empty
]
_refs = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def oracle_scene(cornell_path):
    from oracle import cap_oracle as O
    from oracle import obj_oracle
    g = obj_oracle.load_geometry(cornell_path)
    return O.Scene(g["positions"], g["normals"], g["texcoords"], g["indices"], g["meshes"])


def reference(oracle_scene, bluenoise, case):
    """(planes of the last frame, accumulated sum, rays) of a case by the oracle, computed once per module run"""
    if case not in _refs:
        from oracle import cap_oracle as O
        w, h, first, n, depth = case
        cam = capi.cornell_camera(w, h)
        ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1],
                             cam.focal_length)
        acc, rays = oracle_scene.render_accumulate(ocam, bluenoise, w, h, first, n, depth, threads=8)
        last = oracle_scene.render_frame(ocam, bluenoise, w, h, first + n - 1, depth, threads=8)
        _refs[case] = (last, acc, rays)
    return _refs[case]


def renderer(cornell_path, bluenoise, w, h, shard=(0, 1)):
    r = capi.Renderer(0)
    r.upload_geometry(capi.Geometry(cornell_path))
    r.upload_bluenoise(bluenoise)
    info = r.build_bvh()
    assert info.triangle_count <= 64  # the fused kernels with the scene in LDS
    assert r.debug_get(r.DEBUG_SHADE_TAME) == 1  # ... and tame records: the kernels that have the form
    r.set_resolution(w, h)
    r.set_shard(*shard)
    r.set_camera(capi.cornell_camera(w, h))
    return r


def owned(w, h, shard):
    """Pixels of the tiles shard (index, count) owns: global tile = local tile * count + index, tiles row-major."""
    tx = (w + 7) // 8
    y, x = np.mgrid[0:h, 0:w]
    return ((y // 8) * tx + x // 8) % shard[1] == shard[0]


def assert_planes(r, ref, mask=None):
    for name, kind in PLANES:
        g, o = bits(r.readback(kind)), bits(ref[name])
        bad = (g != o).any(-1)
        if mask is not None:
            bad &= mask
        assert not bad.any(), "%s: %d pixels differ, first (y, x) = %s" % (name, int(bad.sum()), tuple(np.argwhere(bad)[0]))


def assert_clean(s):
    assert s.guard_shade == 0 and s.guard_trace_any == 0 and s.guard_append == 0


def rays_of(s):
    return (s.rays_primary, s.rays_extension, s.rays_shadow)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_f%d_n%d_d%d" % c)
def test_oracle_parity(native_lib, bluenoise, cornell_path, oracle_scene, case):
    w, h, first, n, depth = case
    last, acc, rays = reference(oracle_scene, bluenoise, case)
    assert rays[1] > 0  # paths go on: something sampled
    r = renderer(cornell_path, bluenoise, w, h)
    r.debug_switch("CAP_SAMPLE_TABLE", 1)
    r.render(first, n, depth, capi.RENDER_AOV)  # one batch: the frames are its slots
    assert r.debug_get(r.DEBUG_SAMPLE_TABLE) == 1
    assert_planes(r, last)
    assert np.array_equal(bits(r.readback(capi.BUF_ACCUM_SUM)[..., :3]), bits(acc[..., :3])), "the sum of the %d frames differs" % n
    s = r.stats()
    assert rays_of(s) == rays
    assert_clean(s)
    r.close()


def test_three_shards(native_lib, bluenoise, cornell_path, oracle_scene):
    """16 frames at 104 x 56 (13 x 7 tiles) over three shards, gt = 3 lt + s: every shard's own pixels of the last frame's planes and of
    the sum, and the three shards' rays add up to the oracle's."""
    case = (104, 56, 5, 16, 4)
    w, h, first, n, depth = case
    last, acc, rays = reference(oracle_scene, bluenoise, case)
    total = np.zeros(3, np.int64)
    for index in (1, 0, 2):
        r = renderer(cornell_path, bluenoise, w, h, (index, 3))
        r.debug_switch("CAP_SAMPLE_TABLE", 1)
        r.render(first, n, depth, capi.RENDER_AOV)
        assert r.debug_get(r.DEBUG_SAMPLE_TABLE) == 1
        mask = owned(w, h, (index, 3))
        assert mask.any()
        assert_planes(r, last, mask)
        bad = (bits(r.readback(capi.BUF_ACCUM_SUM)[..., :3]) != bits(acc[..., :3])).any(-1) & mask
        assert not bad.any(), "shard %d: the sum differs at %d owned pixels" % (index, int(bad.sum()))
        s = r.stats()
        assert_clean(s)
        total += rays_of(s)
        r.close()
    assert tuple(int(x) for x in total) == rays


@pytest.mark.parametrize("case", [(136, 72, 3, 1, 4), (104, 56, 5, 9, 4)], ids=lambda c: "%dx%d_f%d_n%d_d%d" % c)
def test_accumulate_only(native_lib, bluenoise, cornell_path, oracle_scene, case):
    """No AOV: bounce 0 takes its CODE form (the first vertex's code in color.w, no direct plane)."""
    w, h, first, n, depth = case
    _, acc, rays = reference(oracle_scene, bluenoise, case)
    r = renderer(cornell_path, bluenoise, w, h)
    r.debug_switch("CAP_SAMPLE_TABLE", 1)
    r.render(first, n, depth, 0)
    assert r.debug_get(r.DEBUG_SAMPLE_TABLE) == 1
    assert np.array_equal(bits(r.readback(capi.BUF_ACCUM_SUM)[..., :3]), bits(acc[..., :3]))
    s = r.stats()
    assert rays_of(s) == rays
    assert_clean(s)
    r.close()


def test_switch_parity_in_one_process(native_lib, bluenoise, cornell_path):
    """The same renders on one context with the table off and on: planes, accumulated sum and every counter of stats() equal as bits."""
    w, h = 136, 72
    r = renderer(cornell_path, bluenoise, w, h)
    shots = {}
    for on in (0, 1, 0, 1):
        r.debug_switch("CAP_SAMPLE_TABLE", on)
        got = []
        for first, n, depth, flags in ((5, 9, 4, capi.RENDER_AOV), (1021, 3, 8, capi.RENDER_AOV), (7, 2, 1, capi.RENDER_AOV), (5, 9, 4, 0)):
            r.accum_reset()
            r.stats_reset()
            r.render(first, n, depth, flags)
            assert r.debug_get(r.DEBUG_SAMPLE_TABLE) == on
            planes = [bits(r.readback(kind)).copy() for _, kind in PLANES] if flags else []
            s = r.stats()
            assert_clean(s)
            counters = tuple(getattr(s, name) for name, kind in s._fields_ if kind is C.c_uint64)  # everything of stats() but the timers
            got.append((planes, bits(r.readback(capi.BUF_ACCUM_SUM)).copy(), counters))
        shots.setdefault(on, []).append(got)
    for a, b in ((shots[0][0], shots[1][0]), (shots[0][1], shots[1][1]), (shots[1][0], shots[1][1])):
        for (pa, sa, ca), (pb, sb, cb) in zip(a, b):
            assert ca == cb
            assert np.array_equal(sa, sb)
            assert len(pa) == len(pb) and all(np.array_equal(x, y) for x, y in zip(pa, pb))
    r.close()


def test_forms_that_have_no_table(native_lib, bluenoise, cornell_path):
    """Depth 0 samples nothing, the tree path and the switch at 0 compute per vertex: the getter says so, and the self-test refuses."""
    r = renderer(cornell_path, bluenoise, 16, 8)
    r.render(3, 1, 0, 0)
    assert r.debug_get(r.DEBUG_SAMPLE_TABLE) == 0
    r.set_traversal(1)
    r.render(3, 1, 2, 0)
    assert r.debug_get(r.DEBUG_SAMPLE_TABLE) == 0
    r.set_traversal(0)
    r.debug_switch("CAP_SAMPLE_TABLE", 0)
    r.render(3, 1, 2, 0)
    assert r.debug_get(r.DEBUG_SAMPLE_TABLE) == 0
    with pytest.raises(capi.CapError):
        r.debug_get(r.DEBUG_SELFTEST_SAMPLE_TABLE)
    r.close()


def test_the_table_itself(native_lib, bluenoise, cornell_path):
    """Every entry of the table a render left, compared on the device with hemisphere_terms of the sample as the kernels without the
    table draw it (by pixel and count).  Frames 5 and 6 at depth 8: count = 125 .. 132 and 150 .. 157, texel offsets 13 .. 4 and 6 .. 13, two
    slots that differ in the offset at every bounce; 8 bounces x 2 slots x 4 096 entries, none may differ in any bit."""
    r = renderer(cornell_path, bluenoise, 16, 8)
    r.debug_switch("CAP_SAMPLE_TABLE", 1)
    r.render(5, 2, 8, 0)
    assert r.debug_get(r.DEBUG_SAMPLE_TABLE) == 1
    v = r.debug_get(r.DEBUG_SELFTEST_SAMPLE_TABLE)
    print("rows compared", v & 0xffffffff, "mismatches", v >> 32)
    assert v & 0xffffffff == 8 * 2
    assert v >> 32 == 0
    r.render(4095, 1, 1, capi.RENDER_AOV)  # one row, k near 4 000
    assert r.debug_get(r.DEBUG_SELFTEST_SAMPLE_TABLE) == 1
    r.close()
