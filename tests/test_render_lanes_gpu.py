"""cap_render's two working sets (lanes) against the same frames on one lane, bit for bit: the AOV frame after a multi-batch
two-lane call (the last batch runs on lane 0, whichever lane the first one took), the single-batch split, working sets that grow
between calls while the accumulation continues, stage timers (one lane, the two-lane batch sizes), and a refused exhaustive
traversal, which must leave the context as it found it.  The one-lane reference is the CAP_NO_TWO_LANES switch."""
import os
import sys

import numpy as np
import pytest

from capsaicin_amd import capi
from test_fallback_kernels_gpu import PLANES, bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H, DEPTH = 96, 64, 3
LANES_USED = capi.Renderer.DEBUG_LANES_USED


@pytest.fixture(scope="module")
def hall():
    import make_sponza_class as gen
    return gen.arrays(0.1, 64)


def make(hall, bluenoise):
    import make_sponza_class as gen
    pos, nrm, uv, idx, meshes, texs = hall
    r = capi.Renderer(0)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    for i, t in enumerate(texs):
        r.upload_texture(i, t)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(W, H)
    r.set_camera(capi.camera_from_config(dict(gen.camera(), sensor_x=0.036), W, H))
    r.set_traversal(1)
    return r


def rays(s):
    assert s.guard_shade == 0 and s.guard_trace_any == 0 and s.guard_append == 0
    return (s.rays_primary, s.rays_extension, s.rays_shadow)


def render(r, n, flags, planes=()):
    """(lanes used, planes read back, accumulated sum, ray counters, stats) of frames 0..n-1 from a cleared accumulation"""
    r.accum_reset()
    r.stats_reset()
    r.render(0, n, DEPTH, flags)
    lanes = r.debug_get(LANES_USED)
    got = [r.readback(k) for k in planes]
    acc = r.readback(capi.BUF_ACCUM_SUM)
    s = r.stats()
    return lanes, got, acc, rays(s), s


@pytest.mark.parametrize("n", [3, 4])  # odd and even batch counts: the first batch on lane 0 and on lane 1
def test_aov_after_a_multi_batch_two_lane_render(native_lib, bluenoise, hall, n):
    r = make(hall, bluenoise)
    r.set_batch_paths(W * H)  # one frame per batch
    lanes, planes, acc, cnt, _ = render(r, n, capi.RENDER_AOV, PLANES)
    assert lanes == 2
    r.debug_switch("CAP_NO_TWO_LANES", 1)
    lanes1, planes1, acc1, cnt1, _ = render(r, n, capi.RENDER_AOV, PLANES)
    assert lanes1 == 1
    for kind, a, b in zip(PLANES, planes, planes1):
        assert np.array_equal(bits(a), bits(b)), kind
    assert np.array_equal(bits(acc), bits(acc1)) and cnt == cnt1
    r.close()


@pytest.mark.parametrize("n", [2, 3])  # 3: halves of 2 and 1 frames
def test_single_batch_split(native_lib, bluenoise, hall, n):
    r = make(hall, bluenoise)
    r.debug_switch("CAP_LANE_SPLIT_MIN", 1)
    lanes, _, acc, cnt, _ = render(r, n, 0)
    assert lanes == 2
    r.debug_switch("CAP_NO_TWO_LANES", 1)
    lanes1, _, acc1, cnt1, _ = render(r, n, 0)
    assert lanes1 == 1
    assert np.array_equal(bits(acc), bits(acc1)) and cnt == cnt1
    r.close()


def test_growth_between_calls(native_lib, bluenoise, hall):
    """both lanes' working sets grow from 1 frame slot to 3 between two calls that add to one accumulation"""
    out = []
    for one_lane in (0, 1):
        r = make(hall, bluenoise)
        r.debug_switch("CAP_LANE_SPLIT_MIN", 1)
        if one_lane:
            r.debug_switch("CAP_NO_TWO_LANES", 1)
        for begin, n in ((0, 2), (2, 6)):
            r.render(begin, n, DEPTH, 0)
            assert r.debug_get(LANES_USED) == (1 if one_lane else 2)
        out.append(r.readback(capi.BUF_ACCUM_SUM))
        rays(r.stats())
        r.close()
    assert np.array_equal(bits(out[0]), bits(out[1]))


@pytest.mark.parametrize("n", [3, 4])
def test_stage_timers_run_on_one_lane(native_lib, bluenoise, hall, n):
    """a stage-timed render launches what the plain one does"""
    r = make(hall, bluenoise)
    r.set_batch_paths(W * H)
    lanes, _, acc, cnt, _ = render(r, n, 0)
    assert lanes == 2
    lanes1, _, acc1, cnt1, s = render(r, n, capi.RENDER_STAGE_TIMERS)
    assert lanes1 == 1
    assert np.array_equal(bits(acc), bits(acc1)) and cnt == cnt1
    assert s.ms_total > 0
    r.close()


def test_refused_exhaustive_traversal_leaves_the_context_usable(native_lib, bluenoise):
    """(the hall at scale 0.1 has 2 652 triangles, which the exhaustive path accepts: this case takes it at 0.15, 5 648 triangles)"""
    import make_sponza_class as gen
    hall = gen.arrays(0.15, 64)
    assert len(hall[3]) // 3 > 4096
    r = make(hall, bluenoise)
    r.set_traversal(2)
    with pytest.raises(capi.CapError):
        r.render(0, 2, DEPTH, 0)
    r.set_traversal(1)
    _, _, acc, cnt, _ = render(r, 2, 0)
    r.close()
    fresh = make(hall, bluenoise)
    _, _, acc1, cnt1, _ = render(fresh, 2, 0)
    fresh.close()
    assert np.array_equal(bits(acc), bits(acc1)) and cnt == cnt1
