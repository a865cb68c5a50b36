"""Bounce 0 of the small-scene path without its constant planes (ShadeArgs::code_in_color): in an accumulate-only render of an
untextured scene bounce 0 writes color = (0, 0, 0, code) and no direct plane, the bounce-0 any-hit launch stores -- not adds -- the
contribution of an unoccluded shadow ray into `direct` and marks the path's code, and the resolve (k_resolve_coded) takes everything
else `direct` would hold from the code.  Cornell box, reference model, depth 4, no CAP_RENDER_AOV (the mode the form exists in); the
accumulator bit for bit against the oracle's sum in frame order, every ray counter, no guard."""
import numpy as np
import pytest

import pair_cull_support as S
from capsaicin_amd import capi

pytestmark = pytest.mark.gpu

DEPTH = 4
FIRST = 3  # first frame of every render
SWITCHES = ("CAP_NO_ALBEDO_IN_W", "CAP_NO_PLANE_CODE")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def box_camera(w, h):
    cam = capi.cornell_camera(w, h)
    return S.Cam(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.focal_length, cam.sensor_size[0], w, h)


def turned_camera(w, h):
    """from outside and to the side of the box: whole tiles of sky, tiles the box's silhouette cuts, tiles inside it"""
    return S.euler_camera((2.5, 1.0, 6.0), 0.5, -0.05, 0.1, w, h, focal=0.035)


def shadow_kinds(geometry, cam, ref, frame):
    """The first vertices of the oracle's frame `ref` by what became of their shadow ray: (lit, occluded by the pair the kernels probe
    first, occluded by something else alone), as pixel counts.  The vertex is rebuilt from the oracle's depth plane along the camera ray
    in float64, and its shadow ray is tested against the probed quad with a margin of 1e-3 of the quad's extent on either side, so
    that a pixel counts as `probe` or `other` only where the rebuilt position cannot decide it wrongly; the rest is in neither."""
    from oracle import cap_oracle as O
    arrays = (geometry["positions"], geometry["normals"], geometry["texcoords"], geometry["indices"], geometry["meshes"])
    pairs, _ = S.fan_records(arrays[0], arrays[3], arrays[4])
    quad = pairs[S.probe_scores(arrays, frame)[1][0]]
    L = np.float64(O.directional_light(frame)[0])
    jx, jy = S.jitter(frame)
    ys, xs = np.mgrid[0:cam.h, 0:cam.w]
    cx, cy = ((xs + jx) / cam.w - 0.5) * float(cam.sx), ((ys + jy) / cam.h - 0.5) * float(cam.sy)
    d = float(cam.focal) * np.float64(cam.forward) + cx[..., None] * np.float64(cam.right) + cy[..., None] * np.float64(cam.up)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    p = np.float64(cam.position) + d * np.float64(ref["normal_depth"][..., 3:4])
    hit = bits(ref["gbuffer_geo"])[..., 3] != capi.MISS
    lit = hit & (ref["direct"][..., :3] != 0).any(-1)
    # the quad as a parallelogram v0 + s e1 + t e3 (e2 = e1 + e3 is its diagonal): where the shadow ray meets its plane
    v0, e1, e3 = np.float64(quad["v0"]), np.float64(quad["e1"]), np.float64(quad["e3"])
    assert np.allclose(np.float64(quad["e2"]), e1 + e3, atol=1e-5)
    n = np.cross(e1, e3)
    t = ((v0 - p) @ n) / (L @ n)
    q = p + t[..., None] * L - v0
    m = np.linalg.inv(np.stack([e1, e3, n], 1))
    s_, t_ = q @ m[0], q @ m[1]
    eps = 1e-3
    inside = (t > 1e-2) & (s_ > eps) & (s_ < 1 - eps) & (t_ > eps) & (t_ < 1 - eps)
    outside = (t < -1e-2) | (s_ < -eps) | (s_ > 1 + eps) | (t_ < -eps) | (t_ > 1 + eps)
    # a dark vertex has a shadow ray only if its surface faces the light: the normal from the oracle's octahedral plane
    # (math_functions.h:36-47 inverted), n . L clearly positive
    o = np.float64(ref["normal_depth"][..., :2]) * 2.0 - 1.0
    nz = 1.0 - np.abs(o[..., 0]) - np.abs(o[..., 1])
    fold = nz < 0
    nx = np.where(fold, (1.0 - np.abs(o[..., 1])) * np.where(o[..., 0] >= 0, 1.0, -1.0), o[..., 0])
    ny = np.where(fold, (1.0 - np.abs(o[..., 0])) * np.where(o[..., 1] >= 0, 1.0, -1.0), o[..., 1])
    nrm = np.stack([nx, ny, nz], -1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    dark = hit & ~lit & (nrm @ L > 1e-3)
    return int(lit.sum()), int((dark & inside).sum()), int((dark & outside).sum())


CASES = {"box 16x8": (16, 8, box_camera), "box 100x52": (100, 52, box_camera), "turned 100x52": (100, 52, turned_camera)}


GEOMETRY = []  # the parsed scene, for shadow_kinds()


@pytest.fixture(scope="module")
def oracle_scene(cornell_path):
    from oracle import cap_oracle as O
    from oracle import obj_oracle
    g = obj_oracle.load_geometry(cornell_path)
    GEOMETRY[:] = [g]
    return O.Scene(g["positions"], g["normals"], g["texcoords"], g["indices"], g["meshes"])


_SUMS, _FRAMES = {}, {}


def oracle_sum(scene, bluenoise, name, n):
    """(sum of frames FIRST .. FIRST + n - 1 in frame order, ray counters), computed once per (case, n)"""
    if (name, n) not in _SUMS:
        w, h, cam = CASES[name]
        _SUMS[name, n] = scene.render_accumulate(cam(w, h).oracle(), bluenoise, w, h, FIRST, n, DEPTH, threads=8)
    return _SUMS[name, n]


def oracle_frame(scene, bluenoise, name):
    if name not in _FRAMES:
        w, h, cam = CASES[name]
        _FRAMES[name] = scene.render_frame(cam(w, h).oracle(), bluenoise, w, h, FIRST, DEPTH, threads=8)
    return _FRAMES[name]


def renderer(cornell_path, bluenoise, name):
    w, h, cam = CASES[name]
    r = capi.Renderer(0)
    r.upload_geometry(capi.Geometry(cornell_path))
    r.upload_bluenoise(bluenoise)
    info = r.build_bvh()
    assert info.triangle_count <= 64  # the fused kernels with the scene in LDS
    r.set_resolution(w, h)
    r.set_camera(cam(w, h).capi())
    return r


def assert_sum(r, acc, what):
    got = r.readback(capi.BUF_ACCUM_SUM)
    bad = (bits(got[..., :3]) != bits(acc[..., :3])).any(-1)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) = %s" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))


def assert_counters(s, rays):
    assert (s.rays_primary, s.rays_extension, s.rays_shadow) == rays
    assert s.guard_shade == 0 and s.guard_trace_any == 0 and s.guard_append == 0


@pytest.mark.parametrize("n", [1, 16])
@pytest.mark.parametrize("name", list(CASES))
def test_sum_of_frames(native_lib, bluenoise, cornell_path, oracle_scene, name, n):
    w, h, _ = CASES[name]
    acc, rays = oracle_sum(oracle_scene, bluenoise, name, n)
    # the kinds of first vertices, on the oracle's planes of the first frame: sky, padding, and by what became of the shadow ray -- lit,
    # occluded by the pair the producer probes, occluded by another pair alone (the any-hit launch's own finding: an entry without a
    # mark).  The box is lit from above through nothing but its open front, so the last kind is rare: the 100 x 52 view from the
    # box's front is the one chosen to hold it and is the only one asked for it; the other views may or may not.
    ref = oracle_frame(oracle_scene, bluenoise, name)
    sky = bits(ref["gbuffer_geo"])[..., 3] == capi.MISS
    n_lit, n_probe, n_other = shadow_kinds(GEOMETRY[0], CASES[name][2](w, h), ref, FIRST)
    assert sky.any() and n_lit > 0 and n_probe > 0
    if name == "box 100x52":
        assert n_other > 0
    padding = ((w + 7) // 8) * ((h + 7) // 8) * 64 - w * h
    assert (padding > 0) == (name != "box 16x8")  # 16 x 8 is two whole tiles; 100 x 52 has partial tiles on two edges
    r = renderer(cornell_path, bluenoise, name)
    r.render(FIRST, n, DEPTH)
    assert_sum(r, acc, "%s, %d frames" % (name, n))
    s = r.stats()
    assert_counters(s, rays)
    if n == 1:
        # the device's own account of the same frame: every lit path and every path another pair occludes was an entry of the any-hit
        # launch (strictly more entries than marks where n_other > 0), and the probe answered shadow rays that never became entries
        assert s.shadow_entries_bounce0 >= n_lit + n_other
        assert s.rays_shadow_bounce0 - s.shadow_entries_bounce0 >= n_probe
    r.close()


def test_stale_direct_entries(native_lib, bluenoise, cornell_path, oracle_scene):
    """Two renders into one context, the second from another camera, without a reset between them: contributions the first left in the
    direct plane lie under pixels that are sky or unlit in the second.  The accumulator must be the sum of the two oracles' sums."""
    n = 16
    a0, rays0 = oracle_sum(oracle_scene, bluenoise, "box 100x52", n)
    a1, rays1 = oracle_sum(oracle_scene, bluenoise, "turned 100x52", n)
    f0, f1 = oracle_frame(oracle_scene, bluenoise, "box 100x52"), oracle_frame(oracle_scene, bluenoise, "turned 100x52")
    lit0 = (f0["direct"][..., :3] != 0).any(-1) & (bits(f0["gbuffer_geo"])[..., 3] != capi.MISS)
    sky1 = bits(f1["gbuffer_geo"])[..., 3] == capi.MISS
    dark1 = ~sky1 & ~(f1["direct"][..., :3] != 0).any(-1)
    assert (lit0 & sky1).any() and (lit0 & dark1).any()  # the same slot (frame) and pixel: the same plane entry
    r = renderer(cornell_path, bluenoise, "box 100x52")
    r.render(FIRST, n, DEPTH)
    r.set_camera(turned_camera(100, 52).capi())
    r.render(FIRST, n, DEPTH)
    # the oracle's sum starts at zero; the context's second render adds its frames one by one onto the first sum
    w, h, cam = CASES["turned 100x52"]
    want = a0[..., :3].copy()
    for f in range(n):
        fr = oracle_scene.render_frame(cam(w, h).oracle(), bluenoise, w, h, FIRST + f, DEPTH, threads=8)
        want = want + fr["combined"][..., :3]
    got = r.readback(capi.BUF_ACCUM_SUM)
    bad = (bits(got[..., :3]) != bits(want)).any(-1)
    assert not bad.any(), "%d pixels differ, first (y, x) = %s" % (int(bad.sum()), tuple(np.argwhere(bad)[0]))
    s = r.stats()
    assert_counters(s, tuple(x + y for x, y in zip(rays0, rays1)))
    r.close()


@pytest.mark.parametrize("switch", SWITCHES + ("CAP_NO_INLINE_PROBE",))
def test_switches_same_bits(native_lib, bluenoise, cornell_path, oracle_scene, switch):
    """The three-plane form (CAP_NO_ALBEDO_IN_W), the two-plane form with the code in direct.w (CAP_NO_PLANE_CODE) and the product's give
    the same accumulator; so does the product's form behind the other bounce-0 any-hit kernel (CAP_NO_INLINE_PROBE: k_trace_any_small)."""
    name, n = "turned 100x52", 16
    acc, rays = oracle_sum(oracle_scene, bluenoise, name, n)
    r = renderer(cornell_path, bluenoise, name)
    r.debug_switch(switch, 1)
    r.render(FIRST, n, DEPTH)
    assert_sum(r, acc, switch)
    assert_counters(r.stats(), rays)
    r.debug_switch(switch, None)
    r.accum_reset()
    r.stats_reset()
    r.render(FIRST, n, DEPTH)
    assert_sum(r, acc, "product after " + switch)
    assert_counters(r.stats(), rays)
    r.close()
