"""The three culls of the fused small-scene kernels on scenes built to defeat them (tests/pair_cull_support.py; the models and the
cases' design are checked on the CPU by tests/test_pair_culls.py):
  N  the next-event pair cull of the EXT model (ctx_scene.hip update_nee_pairs): CAP_DEBUG_NEE_PAIRS equals the model's counts;
  C  the camera pair cull of bounce 0 (small_scene.hip stage_camera_pairs, the gate in ctx_render.hip cull_camera_pairs): CAP_DEBUG_CAMERA_CULL equals the model's gate;
  P  the occluder-first probes of the reference model and the EXT model's inline next-event rays.
Every case renders two frames of depth 3 with the cull on and equals the oracle bit for bit in every plane and the three ray counters;
the same context then renders with the switch flipped and gives the same bits."""
import numpy as np
import pytest

import pair_cull_support as S
from capsaicin_amd import capi

pytestmark = pytest.mark.gpu

PLANES = (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("direct", capi.BUF_DIRECT), ("indirect", capi.BUF_INDIRECT),
          ("normal_depth", capi.BUF_NORMAL_DEPTH))
NEE, CAMERA, PROBE = S.NEE_NAMES, S.CAMERA_NAMES, S.PROBE_NAMES  # names: a case is built when its test runs


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


def renderer(case, ext, bluenoise):
    r = capi.Renderer(0)
    r.upload_scene(*case.arrays)
    if ext:
        r.upload_materials(case.mats)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(case.cam.w, case.cam.h)
    r.set_camera(case.cam.capi())
    return r


def check_frames(r, case, ext, bluenoise, what):
    """both frames against the oracle: every plane (and `combined` for EXT) and the ray counters.  AUTO traversal: at most 64
    triangles -> the fused kernels."""
    for frame in case.frames:
        ref = S.reference(case, ext, frame, bluenoise)
        r.stats_reset()
        r.render(frame, 1, S.DEPTH, capi.RENDER_AOV | (capi.RENDER_EXT_MATERIALS if ext else 0))
        for name, kind in PLANES + ((("combined", capi.BUF_COMBINED),) if ext else ()):
            assert_same(r.readback(kind), ref[name], "%s%s, %s: %s (frame %d)" % (case.name, ", EXT" if ext else "", what, name, frame))
        s = r.stats()
        assert (s.rays_primary, s.rays_extension, s.rays_shadow) == ref["rays"], (case.name, what, frame)
        assert s.guard_shade == 0 and s.guard_append == 0


def nee_pairs(r):
    v = r.debug_get(r.DEBUG_NEE_PAIRS)
    return v >> 32, v & 0xFFFFFFFF


def check_nee(r, case, bluenoise):
    """the list as the model says, the oracle's bits with it, the same bits without it (the list is rebuilt by build_bvh)"""
    counts = S.nee_counts(case.arrays, case.mats)
    assert nee_pairs(r) == counts, case.name
    check_frames(r, case, True, bluenoise, "next-event cull on")
    r.debug_switch("CAP_NO_NEE_PAIR_CULL", 1)
    r.build_bvh()
    assert nee_pairs(r) == (counts[1], counts[1])
    check_frames(r, case, True, bluenoise, "next-event cull off")
    r.debug_switch("CAP_NO_NEE_PAIR_CULL", None)
    r.build_bvh()
    assert nee_pairs(r) == counts


@pytest.mark.parametrize("name", NEE)
def test_nee_pair_cull(native_lib, bluenoise, name):
    """N1 .. N5.  N3 at 0.99e-6 D is the case the rule's first tolerance got wrong: the wall, culled, no longer shadowed the decal.
    At 0.5 and 0.9 of the tolerance the rule has now the wall is culled with the decal outside its plane -- the case its proof covers."""
    case = S.case(name)
    r = renderer(case, True, bluenoise)
    check_nee(r, case, bluenoise)
    if case.name.startswith("N1"):
        assert r.debug_get(r.DEBUG_CAMERA_CULL) == 1  # the Cornell camera
    r.close()


def test_nee_pair_cull_follows_a_refit(native_lib, bluenoise):
    """N6: update_vertices + refit_bvh move the lamp from the middle of the room to half a delta under the ceiling and back; the
    ceiling's pair leaves the list, returns and leaves again"""
    mid, near = S.cases(S.REFIT_NAMES)
    r = renderer(mid, True, bluenoise)
    for case in (mid, near, mid):
        r.update_vertices(positions=case.arrays[0])
        r.refit_bvh()
        check_nee(r, case, bluenoise)  # the counts right after the refit first; its build_bvh calls rebuild from the moved vertices
    r.close()


@pytest.mark.parametrize("name", CAMERA)
def test_camera_pair_cull(native_lib, bluenoise, name):
    """C1 .. C7, both shading models.  C4's cameras pass every 1e-4 term of the gate as it was and lose the quad's hits in the tiles
    next to it with the cull on; the gate tied to the pad turns the cull off for them.  C7's are just inside the gate: cull on."""
    case = S.case(name)
    for ext in (False, True):
        r = renderer(case, ext, bluenoise)
        check_frames(r, case, ext, bluenoise, "camera cull as gated")
        assert r.debug_get(r.DEBUG_CAMERA_CULL) == case.expect["gate"] == S.camera_gate(case.cam)[0]
        r.debug_switch("CAP_NO_CAMERA_CULL", 1)
        check_frames(r, case, ext, bluenoise, "camera cull off")
        assert r.debug_get(r.DEBUG_CAMERA_CULL) == 0
        r.debug_switch("CAP_NO_CAMERA_CULL", None)
        r.render(case.frames[0], 1, 0, 0)
        assert r.debug_get(r.DEBUG_CAMERA_CULL) == case.expect["gate"]
        r.close()


REF_SETTINGS = ([[("CAP_NO_INLINE_PROBE", 1)], [("CAP_NO_WAVE_RING", 1)], [("CAP_NO_ANY_PROBE", 1)], [("CAP_NO_INLINE_PROBE", 1), ("CAP_NO_ANY_PROBE", 1)]] +
                [[("CAP_ANY_PROBE", n)] for n in (0, 2, 4)] + [[("CAP_NO_INLINE_PROBE", 1), ("CAP_ANY_PROBE", n)] for n in (0, 2, 4)])
EXT_SETTINGS = [[("CAP_NO_INLINE_NEE", 1)], [("CAP_NO_INLINE_NEE", 1), ("CAP_NO_NEE_PAIR_CULL", 1)]]


@pytest.mark.parametrize("name,ext", PROBE, ids=["%s%s" % (n, ", EXT" if e else "") for n, e in PROBE])
def test_probe_switches(native_lib, bluenoise, name, ext):
    """the producer-side probe, the per-wave ring, the any-hit kernel's own probe with 0, 1 (default), 2 and 4 pairs probed first, the
    EXT model's inline next-event rays: one context, every setting the oracle's bits.  32 pairs, one pair, none; two pairs with
    bit-equal probe scores on top of the order (frame 0); a scene whose probe answers almost nothing."""
    case = S.case(name)
    r = renderer(case, ext, bluenoise)
    check_frames(r, case, ext, bluenoise, "product's choice")
    for setting in (EXT_SETTINGS if ext else REF_SETTINGS):
        for name, value in setting:
            r.debug_switch(name, value)
        if ext:
            r.build_bvh()
        check_frames(r, case, ext, bluenoise, " ".join("%s=%d" % s for s in setting))
        for name, _ in setting:
            r.debug_switch(name, None)
    r.close()
