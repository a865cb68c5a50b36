"""The reconstruction chain (post.hip) on crafted planes and sizes against the oracle's chain, bit for bit, every frame with the
histories carried along -- the cases of tests/post_planes_support.py, each of which tests/test_post_planes.py proves to reach the
path it is named after -- plus closed forms on the device that do not go through the oracle, and two checks that tie the crafted
planes' layout and the render's own tile-ordered path (cap_post_frame) to them."""
import numpy as np
import pytest

import post_planes_support as S
from capsaicin_amd import capi, tiles
from test_oracle_post import camera, wall_planes

pytestmark = pytest.mark.gpu

F = np.float32
_GPU = {}


def gpu_outputs(name):
    """The device's frames of a case, computed once and shared by the tests that read them."""
    if name not in _GPU:
        c = S.CASES[name]()
        r = capi.Renderer(0)
        r.set_resolution(c.w, c.h)
        try:
            _GPU[name] = S.run_gpu(r, c.settings, c.frames)
        finally:
            r.close()
    return _GPU[name]


def assert_same_bits(got, want, what):
    for f, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        bad = (S.bits(a) != S.bits(b)).any(-1)
        if bad.any():
            y, x = (int(v) for v in np.argwhere(bad)[0])
            raise AssertionError("%s frame %d: %d pixels differ, first at (x %d, y %d) in 32x8 tile (%d, %d): got %s want %s"
                                 % (what, f, int(bad.sum()), x, y, x // 32, y // 8, a[y, x], b[y, x]))
    assert len(got) == len(want)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_bit_parity(native_lib, name):
    got = gpu_outputs(name)
    assert all(np.all(np.isfinite(g)) for g in got)
    assert_same_bits(got, S.oracle_outputs(name), name)


@pytest.mark.parametrize("name", sorted(n for n in S.CASES if n.startswith("e-sky")))
def test_sky_pixels_pass_through_on_the_device(native_lib, name):
    """The closed form of tests/test_post_planes.py::test_sky_pixels_pass_through, on the device's own output."""
    c = S.CASES[name]()
    s = capi.PostSettings(**c.settings)
    exact = S.centre_survives_uv(c.w, c.h)
    for (f, _, _, p), out in zip(c.frames, gpu_outputs(name)):
        sky = S.is_background(p["normal_depth"][..., 3]) & exact
        ind = S.remove_fireflies(p["indirect"][..., :3])
        want = {0: ind * p["albedo"][..., :3] + p["direct"][..., :3], 1: p["direct"][..., :3], 2: ind, 3: np.zeros_like(ind)}[s.output]
        assert sky.any()
        assert np.array_equal(S.bits(out[..., :3])[sky], S.bits(want.astype(F))[sky]), (name, f)
        assert np.all(out[..., 3] == 1.0)


@pytest.mark.parametrize("settings", [dict(), dict(gather=0), dict(denoise=0), dict(eaw5=0)])
def test_constant_input_is_a_fixed_point_on_the_device(native_lib, settings):
    """tests/test_oracle_post.py::test_constant_input_is_a_fixed_point with its bounds (and their reasons), on the device."""
    w, h = 48, 32
    cam = camera(w, h)
    planes = wall_planes(w, h, cam, value=0.37)
    r = capi.Renderer(0)
    r.set_resolution(w, h)
    outs = S.run_gpu(r, settings, [(f, cam, cam, planes) for f in range(5)])
    r.close()
    for f, out in enumerate(outs):
        assert np.all(np.isfinite(out))
        assert np.abs(out[..., :3] - 0.37).max() < 5e-3, f
    assert np.abs(outs[-1][..., :3] - 0.37).max() < 1.5e-3


def test_history_cut_on_the_device(native_lib):
    """tests/test_oracle_post.py::test_history_length_and_reset_on_camera_cut on the device: the frame after the cut equals a first frame."""
    from oracle import cap_oracle as O
    w, h = 32, 24
    cam = camera(w, h)
    far = O.make_camera((100.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.036, 0.036 * h / w, 0.035)
    rng = np.random.default_rng(3)
    seq = [wall_planes(w, h, cam, rng=rng) for _ in range(4)]
    r = capi.Renderer(0)
    r.set_resolution(w, h)
    outs = S.run_gpu(r, dict(denoise=0, gather=0), [(f, cam, far if f == 3 else cam, seq[f]) for f in range(4)])
    r.close()
    # no history is usable: accumulate resets, TAA writes the bilinear tap of the combined image = the image itself
    want = seq[3]["indirect"][..., :3] * seq[3]["albedo"][..., :3] + seq[3]["direct"][..., :3]
    assert np.array_equal(outs[3][:-1, :-1, :3], want[:-1, :-1])
    assert not np.array_equal(outs[2][:-1, :-1, :3], (seq[2]["indirect"][..., :3] * seq[2]["albedo"][..., :3])[:-1, :-1])  # history was in use


def cornell(bluenoise, cornell_path, w, h):
    r = capi.Renderer(0)
    r.upload_geometry(capi.Geometry(cornell_path))
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(w, h)
    return r


def resolved_tiles(r):
    import torch
    t = torch.empty(r.aov_tile_buffer_floats(), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # the renderer runs on its own stream
    r.resolve_aov_tiles(t.data_ptr())
    r.sync()
    return t


def test_crafted_planes_mean_what_the_renders_planes_mean(native_lib, bluenoise, cornell_path):
    """run_gpu's upload (tiles.extract of four row-major planes, concatenated in the chain's order) is the buffer the product
    itself hands to cap_post_frame_gathered: cap_resolve_aov_tiles of a rendered frame equals it in every slot that maps to a pixel
    (padding slots carry no pixel; assembly never reads them).  All four planes have a row-major readback."""
    w, h = 70, 23
    r = cornell(bluenoise, cornell_path, w, h)
    r.set_camera(capi.cornell_camera(w, h))
    r.render(0, 1, 2, capi.RENDER_AOV)
    n = tiles.padded_pixels(w, h, 1)
    got = resolved_tiles(r).cpu().numpy().reshape(4, n, 4)
    _, _, valid = tiles.pixel_table(w, h, 0, 1)
    assert valid.sum() == w * h
    for k, kind in enumerate((capi.BUF_INDIRECT, capi.BUF_DIRECT, capi.BUF_ALBEDO, capi.BUF_NORMAL_DEPTH)):
        img = r.readback(kind)
        assert np.abs(img).sum() > 0
        want = tiles.extract(img, 0, 1)
        assert np.array_equal(S.bits(got[k][valid]), S.bits(want[valid])), S.PLANE_ORDER[k]
        assert np.array_equal(S.bits(tiles.assemble([got[k]], w, h)), S.bits(img))
    r.close()


def quad_scene(w, h):
    """One quad facing the camera of `quad_camera`, half the view wide and high: geometry in the middle, sky all around."""
    x, y = 1.2, 1.2 * h / w
    tris = np.float32([[[-x, -y, 0], [x, -y, 0], [x, y, 0]], [[-x, -y, 0], [x, y, 0], [-x, y, 0]]])
    pos = tris.reshape(-1, 3)
    nrm = np.tile(np.float32([0, 0, 1]), (6, 1))
    return pos, nrm, np.zeros((6, 2), F), np.arange(6, dtype=np.uint32), np.uint32([[6, 0, 6, 0, 0, 0xFFFFFFFF, 0, 0]])


def quad_camera(w, h, dx):
    cam = capi.CameraData()
    cam.position[:] = (dx, 0.0, 4.0)
    cam.forward[:] = (0, 0, -1)
    cam.right[:] = (-1, 0, 0)
    cam.up[:] = (0, 1, 0)
    cam.focal_length = 0.03
    cam.sensor_size[0] = 0.036
    cam.sensor_size[1] = F(0.036) * (F(h) / F(w))
    return cam


@pytest.mark.parametrize("w,h", [(1, 1), (9, 3), (33, 9), (7, 130)])
def test_tiled_path_at_sizes_with_sky(native_lib, bluenoise, w, h):
    """cap_post_frame takes the render's tile-ordered planes (TILED Gather, Combine reading tiled direct and albedo), which crafted
    planes cannot reach: a rendered quad with a sky border, four frames with a small translation, depth 1.  cap_post_frame,
    cap_post_frame_gathered with ONE shard on the resolved tiles, and the oracle's chain on the oracle's render agree bit for bit."""
    from oracle import cap_oracle as O
    arrays = quad_scene(w, h)
    r = capi.Renderer(0)
    r.upload_scene(*arrays)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(w, h)
    sc = O.Scene(*arrays)
    chain = O.PostChain(w, h)
    cams = [quad_camera(w, h, 0.01 * k) for k in range(4)]
    gs, os_ = capi.PostSettings(), O.PostSettings()
    want, sky_seen, hit_seen = [], False, False
    for f, cam in enumerate(cams):
        prev = cams[max(f - 1, 0)]
        ref = sc.render_frame(S.oracle_cam(cam), bluenoise, w, h, f, 1, threads=4)
        want.append(chain.frame(os_, f, S.oracle_cam(cam), S.oracle_cam(prev), ref))
        d = ref["normal_depth"][..., 3]
        sky_seen |= bool(S.is_background(d).any())
        hit_seen |= bool((~S.is_background(d)).any())
    assert hit_seen and (sky_seen or (w, h) == (1, 1))

    def sequence(gathered):
        out = []
        r.post_reset()
        for f, cam in enumerate(cams):
            prev = cams[max(f - 1, 0)]
            r.set_camera(cam)
            r.render(f, 1, 1, capi.RENDER_AOV)
            if gathered:
                t = resolved_tiles(r)
                r.post_frame_gathered(gs, f, prev, t.data_ptr(), 1)
            else:
                r.post_frame(gs, f, prev)
            out.append(r.post_readback())
        return out

    assert_same_bits(sequence(False), want, "cap_post_frame %dx%d" % (w, h))
    assert_same_bits(sequence(True), want, "cap_post_frame_gathered(1) %dx%d" % (w, h))
    r.close()
