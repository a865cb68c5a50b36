"""The HIP side of the EXT shading model on the scenes of tests/ext_radiometry_support.py: bit for bit the oracle in every plane and
ray counter (the far furnace's materials, the lamp scene's three light-table paths, light tables built against the pick), and the
accumulated mean of cap_render against the float64 radiometry with the bounds of tests/test_ext_radiometry.py, where the oracle itself
is held to it."""
import numpy as np
import pytest

import ext_radiometry_support as R
from capsaicin_amd import capi

pytestmark = pytest.mark.gpu
B_FURNACE, B_LAMP_TOTAL, B_LAMP_BAND = R.B_FURNACE, R.B_LAMP_TOTAL, R.B_LAMP_BAND

PLANES = (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("direct", capi.BUF_DIRECT), ("albedo", capi.BUF_ALBEDO),
          ("normal_depth", capi.BUF_NORMAL_DEPTH), ("indirect", capi.BUF_INDIRECT), ("combined", capi.BUF_COMBINED))
W, H = 64, 48
FRAMES, DEPTHS = (0, 7, 1023), (1, 8)
# (traversal, switches): auto, tree, exhaustive; the binary tree's kernels; next-event rays through the queue and the any-hit kernel
SETTINGS = ((0, ()), (1, ()), (2, ()), (1, ("CAP_NO_WIDE8",)), (0, ("CAP_NO_WIDE8",)), (0, ("CAP_NO_INLINE_NEE",)), (2, ("CAP_NO_INLINE_NEE",)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, ref, what):
    g, r = bits(got), bits(ref)
    if not np.array_equal(g, r):
        bad = np.argwhere((g != r).any(-1))
        msg = ["%s: %d pixels differ" % (what, len(bad))]
        for b in bad[:6]:
            msg.append("  (y,x)=%s gpu=%s oracle=%s" % (tuple(b), got[tuple(b)], ref[tuple(b)]))
        raise AssertionError("\n".join(msg))


def renderer(scene, bluenoise):
    r = capi.Renderer(0)
    r.upload_scene(*scene.arrays)
    r.upload_materials(scene.mats)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(scene.cam.w, scene.cam.h)
    r.set_camera(scene.cam.capi())
    return r


def check_frame(r, scene, bluenoise, frame, depth, what):
    ref = R.oracle_frame(scene, bluenoise, frame, depth)
    r.accum_reset()
    r.stats_reset()
    r.render(frame, 1, depth, capi.RENDER_AOV | capi.RENDER_EXT_MATERIALS)
    for name, kind in PLANES:
        assert_same(r.readback(kind), ref[name], "%s, %s: %s (frame %d, depth %d)" % (scene.name, what, name, frame, depth))
    s = r.stats()
    assert (s.rays_primary, s.rays_extension, s.rays_shadow) == ref["rays"], (scene.name, what, frame, depth)
    assert s.guard_shade == 0 and s.guard_append == 0 and s.guard_trace_any == 0
    return s


def check_path(r, scene, s, traversal, switches):
    """that the path meant is the path taken, from the launch counters: the small-scene kernels shade inside the launch that traces
    (no stand-alone shade launch) and, unless switched off, trace the next-event rays where they are made (nothing queued); the tree
    path has a shade launch per bounce >= 1 and the 8-wide view unless CAP_NO_WIDE8"""
    small = traversal == 2 or (traversal == 0 and scene.total <= 64)
    if small:
        assert s.launches_shade == 0, (scene.name, traversal, switches)
        if "CAP_NO_INLINE_NEE" in switches:
            assert s.launches_trace_any > 0 and s.shadow_entries > 0
        else:
            assert s.launches_trace_any == 0 and s.shadow_entries == 0
    else:
        assert s.launches_shade > 0 and s.launches_trace_any > 0 and s.shadow_entries > 0, (scene.name, traversal, switches)
        if "CAP_NO_WIDE8" in switches:
            assert r.debug_get(r.DEBUG_WIDE_IN_USE) == 0
        elif scene.total > 64:
            assert r.debug_get(r.DEBUG_WIDE_IN_USE) == 1


def check_settings(scene, bluenoise, settings, frames, depths):
    r = renderer(scene, bluenoise)
    for traversal, switches in settings:
        r.set_traversal(traversal)
        for name in switches:
            r.debug_switch(name, 1)
        r.build_bvh()
        for depth in depths:
            for frame in frames:
                s = check_frame(r, scene, bluenoise, frame, depth, "traversal %d %s" % (traversal, " ".join(switches)))
                if depth:
                    check_path(r, scene, s, traversal, switches)
        for name in switches:
            r.debug_switch(name, None)
    r.close()


@pytest.mark.parametrize("name", list(R.FURNACE_MATERIALS) + ["ggx r0", "black"])
def test_far_furnace_parity(native_lib, bluenoise, name):
    """every plane and the three ray counters, frames 0, 7 and 1023, depths 1 and 8, under each of SETTINGS: the materials of the CPU
    test plus roughness 0 (the alpha clamp) and kd = ks = 0 (the path ends at the plate).  18 triangles: the LDS light table."""
    scene = R.far_furnace(name, W, H)
    assert scene.emissive == 12 and scene.total == 18
    check_settings(scene, bluenoise, SETTINGS, FRAMES, DEPTHS)


@pytest.mark.parametrize("size", list(R.LAMP_SIZES))
def test_lamp_scene_parity(native_lib, bluenoise, size):
    """the same on the lamp scene's three sizes: 28 emissive triangles of 32 (small-scene kernels, light table in LDS), 40 of 44 (the
    same kernels, more lights than the LDS table holds: the global table), 304 of 308 (tree path under auto).  Two lamps that differ in
    ke, with a mesh that emits nothing between them and zero-area emissive triangles."""
    scene = R.lamp_scene(size, w=W, h=H)
    assert (scene.emissive <= 32) == (size == "lds table") and (scene.total <= 64) == (size != "tree")
    check_settings(scene, bluenoise, SETTINGS, FRAMES, DEPTHS)


def test_lamp_scene_zero_channels_parity(native_lib, bluenoise):
    """ke with a zero channel in either lamp, auto and tree"""
    scene = R.lamp_scene("lds table", (4.0, 0.0, 1.0), (0.0, 3.0, 9.0), W, H)
    check_settings(scene, bluenoise, SETTINGS[:2], FRAMES, (1,))


@pytest.mark.parametrize("length", R.HARD_LENGTHS)
def test_light_pick_on_hard_tables(native_lib, bluenoise, length):
    """The binary search of shade_vertex_ext against the oracle's linear scan, depth 0: tables of 1, 2, 31, 32, 33 and 64 entries whose
    areas span six orders of magnitude, with zero-area entries first, in a run of three and as the last two -- equal prefix
    sums.  The table is what the support module says it is."""
    scene = R.hard_table_scene(length)
    cdf, total = R.light_table(scene)
    assert len(cdf) == length and total > 0
    if length > 2:
        live = np.diff(np.concatenate([[np.float32(0)], cdf]))
        assert int((live == 0).sum()) >= 6 and live[live > 0].max() / live[live > 0].min() > 1e5
    check_settings(scene, bluenoise, SETTINGS[:3], FRAMES, (0,))


@pytest.mark.parametrize("name", list(R.FURNACE_MATERIALS))
def test_far_furnace_accumulated_mean(native_lib, bluenoise, name):
    """cap_render over 64 frames in two batches, depth 1, 256 x 256: the plate emits nothing, so the accumulated mean on it is
    direct + indirect = 1.5 E(mu).  Plate-wide and over the halves of the plate by n.wo, per channel, B = 3 % as on the CPU (the oracle's
    own figures there: the worst of them is 1.25 %).  For the Lambert plate the mean is also the oracle's, pixel by pixel, up to
    the rounding of the fp32 sum."""
    scene = R.far_furnace(name)
    w, h = scene.cam.w, scene.cam.h
    r = renderer(scene, bluenoise)
    r.set_batch_paths(32 * w * h)
    r.render(0, R.FURNACE_FRAMES, 1, capi.RENDER_EXT_MATERIALS)
    mean = np.float64(r.readback(capi.BUF_ACCUM_MEAN)[..., :3])
    s = r.stats()
    assert s.frames == R.FURNACE_FRAMES and s.guard_shade == 0 and s.guard_append == 0
    r.close()
    ref = R.oracle_means(R.far_furnace("lambert"), bluenoise, R.FURNACE_FRAMES, 1)  # the plate's pixels are the same for every material
    on = ref["on0"]
    dev = R.furnace_deviations(mean / 1.5, mean / 3.0, on, name)
    print(name, {k: np.round(100 * v, 2).tolist() for k, v in dev.items() if k.startswith("direct")})
    for key in ("direct", "direct_lo", "direct_hi"):
        assert np.abs(dev[key]).max() < B_FURNACE, (name, key, dev[key])
    if name == "lambert":
        assert np.allclose(mean, ref["direct"] + ref["indirect"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("size", list(R.LAMP_SIZES))
def test_lamp_scene_accumulated_mean(native_lib, bluenoise, size):
    """cap_render over 16 frames in two batches, depth 0, 192 x 144: the floor emits nothing, so the accumulated mean on it is
    `direct`; floor-wide sum and band sums against the lamps' integrals with the CPU test's bounds"""
    scene = R.lamp_scene(size)
    w, h = scene.cam.w, scene.cam.h
    r = renderer(scene, bluenoise)
    r.set_batch_paths(8 * w * h)
    r.render(0, R.LAMP_FRAMES, 0, capi.RENDER_EXT_MATERIALS)
    mean = np.float64(r.readback(capi.BUF_ACCUM_MEAN)[..., :3])
    s = r.stats()
    assert s.frames == R.LAMP_FRAMES and s.guard_shade == 0 and s.guard_append == 0
    r.close()
    on = R.oracle_means(R.lamp_scene("lds table"), bluenoise, R.LAMP_FRAMES, 0)["on0"]  # the floor's pixels are the same for every size
    dev = R.lamp_deviations(mean, on)
    print(size, np.round(100 * dev["total"], 2).tolist(), np.round(100 * dev["bands"], 2).tolist())
    assert np.abs(dev["total"]).max() < B_LAMP_TOTAL and np.abs(dev["bands"]).max() < B_LAMP_BAND, dev
