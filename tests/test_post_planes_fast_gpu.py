"""CapPostSettings::fast_weights on the crafted planes of tests/post_planes_support.py.  The mode is not bit-comparable with the
oracle, and no fixed tolerance carries over to arbitrary planes: a relative change of 2^-16 of the colour inputs already moves the
EXACT chain's output by more than the header's stated median.  So the bound is the reference's own sensitivity, case by case and
frame by frame (S.sensitivity: the oracle on perturbed colours, four draws), with e = |a - b| / (|b| + 1e-3) per colour channel:

    Q50, Q99, Qmax of e(fast, exact)  <=  4 * max(S50, S99, Smax of e(perturbed exact, exact), 2^-20)   respectively.

2^-16 is the size class of what the project states for the two modes' weights (about 1e-5: v_exp_f32 / v_log_f32 / v_rcp_f32 at
1 ulp behind a 128-fold exponent, fused instead of separate roundings).  To first order a relative error delta in the weights of a
normalised sum of non-negative colours moves it by at most delta times the spread of the colours in the window, the same delta on
the colours by up to delta times their maximum, and the perturbed run goes through the same later passes and histories, TAA's
variance clipping included.  The factor 4 covers the first-order argument, up to three weight factors per tap, and that four draws
are a sample and not a supremum.  Neither number comes from the fast mode's output.  Frames that are too ill-conditioned for their
maximum to mean anything, and images too small for quantiles, are judged as tests/test_post_planes.py states and proves.

Then what needs no tolerance, in fast mode on the device: sky pass-through, the history cut, the constant fixed point, and the
tiled entry point against the gathered one, bit for bit."""
import numpy as np
import pytest

import post_planes_support as S
from capsaicin_amd import capi
from test_oracle_post import camera, wall_planes
from test_post_planes_gpu import assert_same_bits, quad_camera, quad_scene, resolved_tiles

pytestmark = pytest.mark.gpu

F = np.float32
_FAST = {}


def fast_outputs(name):
    """The device's frames of a case in fast mode (a fresh Renderer, histories carried), computed once and shared."""
    if name not in _FAST:
        c = S.CASES[name]()
        r = capi.Renderer(0)
        r.set_resolution(c.w, c.h)
        try:
            _FAST[name] = S.run_gpu(r, dict(c.settings, fast_weights=1), c.frames)
        finally:
            r.close()
    return _FAST[name]


def judge(name, got):
    """-> (lines of figures, failures) of a case's fast frames against the budgets."""
    c, exact, s = S.CASES[name](), S.oracle_outputs(name), S.sensitivity(name)
    assert len(got) == len(exact) == len(s)
    q = np.array([S.quantiles(S.rel_err(g, b)) for g, b in zip(got, exact)])
    bound = S.BUDGET * np.maximum(s, S.S_FLOOR)
    lines, fails = [], []
    if c.w * c.h < S.SMALL_IMAGE:
        qmax, smax = q[:, 2].max(), S.BUDGET * max(s[:, 2].max(), S.S_FLOOR)
        lines.append("%s whole sequence: Qmax %.3e bound %.3e ratio to S %.2f" % (name, qmax, smax, S.BUDGET * qmax / smax))
        if not qmax <= smax:
            fails.append(lines[-1])
        return lines, fails
    for f in range(len(got)):
        judged = [0, 1] if s[f, 2] > S.ILL_CONDITIONED else [0, 1, 2]
        lines.append("%s frame %2d: Q %.3e %.3e %.3e  bound %.3e %.3e %.3e  Q/S %.2f %.2f %.2f%s" % (
            (name, f) + tuple(q[f]) + tuple(bound[f]) + tuple(S.BUDGET * q[f] / bound[f]) + ("" if len(judged) == 3 else "  (max not judged)",)))
        if not all(q[f, i] <= bound[f, i] for i in judged):
            fails.append(lines[-1])
    return lines, fails


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_fast_within_the_exact_chains_sensitivity(native_lib, name):
    """Finite, and every judged quantile inside its budget; the figures of every frame are printed before the assertion.
    Measured on the device ("Reconstruction chain", has the table): the largest Q / max(S, 2^-20) over all cases is
    0.77 / 1.94 / 1.87 for the median / 99th percentile / maximum, against the budget's 4."""
    got = fast_outputs(name)
    assert all(np.all(np.isfinite(g)) for g in got)
    lines, fails = judge(name, got)
    print("\n".join(lines))
    assert not fails, "\n".join(fails)


def test_the_switch_does_something(native_lib):
    """It IS another arithmetic: in every case with 256 or more geometry pixels and the combined output, equal bits in every frame
    would mean the switch is not wired."""
    judged = 0
    for name in sorted(S.CASES):
        c = S.CASES[name]()
        nonsky = min(int((~S.is_background(fr[3]["normal_depth"][..., 3])).sum()) for fr in c.frames)
        if nonsky < 256 or S.oracle_settings(c.settings).output != 0:
            continue
        judged += 1
        assert any((S.bits(g) != S.bits(b)).any() for g, b in zip(fast_outputs(name), S.oracle_outputs(name))), name
    assert judged >= 30


@pytest.mark.parametrize("name", sorted(n for n in S.CASES if n.startswith("e-sky")) + ["a-size-70x23", "g-camera-yaw"])
def test_sky_pixels_pass_through_in_fast_mode(native_lib, name):
    """test_post_planes_gpu.py::test_sky_pixels_pass_through_on_the_device's closed form, bit for bit, in fast mode: every pass
    returns a background pixel unchanged in both modes, and where the pixel centre survives the UV round trip the fast mode's texel
    is what the exact bilinear tap is.  Also on the scattered sky texels of two cases that are mostly geometry."""
    c = S.CASES[name]()
    s = S.oracle_settings(c.settings)
    assert s.denoise
    exact = S.centre_survives_uv(c.w, c.h)
    for (f, _, _, p), out in zip(c.frames, fast_outputs(name)):
        sky = S.is_background(p["normal_depth"][..., 3]) & exact
        ind = S.remove_fireflies(p["indirect"][..., :3])
        want = {0: ind * p["albedo"][..., :3] + p["direct"][..., :3], 1: p["direct"][..., :3], 2: ind, 3: np.zeros_like(ind)}[s.output]
        assert sky.any()
        assert np.array_equal(S.bits(out[..., :3])[sky], S.bits(want.astype(F))[sky]), (name, f)
        assert np.all(out[..., 3] == 1.0)


@pytest.mark.parametrize("settings", [dict(), dict(gather=0), dict(denoise=0), dict(eaw5=0)])
def test_constant_input_is_a_fixed_point_in_fast_mode(native_lib, settings):
    """tests/test_oracle_post.py::test_constant_input_is_a_fixed_point with its bounds (and their reasons), in fast mode."""
    w, h = 48, 32
    cam = camera(w, h)
    planes = wall_planes(w, h, cam, value=0.37)
    r = capi.Renderer(0)
    r.set_resolution(w, h)
    outs = S.run_gpu(r, dict(settings, fast_weights=1), [(f, cam, cam, planes) for f in range(5)])
    r.close()
    for f, out in enumerate(outs):
        assert np.all(np.isfinite(out))
        assert np.abs(out[..., :3] - 0.37).max() < 5e-3, f
    assert np.abs(outs[-1][..., :3] - 0.37).max() < 1.5e-3


def test_history_cut_in_fast_mode(native_lib):
    """test_post_planes_gpu.py::test_history_cut_on_the_device in fast mode: the frame after the cut is the frame itself (the fast
    Accumulate and TAA take the texel where the exact ones take a bilinear tap with weights of 0)."""
    from oracle import cap_oracle as O
    w, h = 32, 24
    cam = camera(w, h)
    far = O.make_camera((100.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.036, 0.036 * h / w, 0.035)
    rng = np.random.default_rng(3)
    seq = [wall_planes(w, h, cam, rng=rng) for _ in range(4)]
    r = capi.Renderer(0)
    r.set_resolution(w, h)
    outs = S.run_gpu(r, dict(denoise=0, gather=0, fast_weights=1), [(f, cam, far if f == 3 else cam, seq[f]) for f in range(4)])
    r.close()
    want = seq[3]["indirect"][..., :3] * seq[3]["albedo"][..., :3] + seq[3]["direct"][..., :3]
    assert np.array_equal(outs[3][:-1, :-1, :3], want[:-1, :-1])
    assert not np.array_equal(outs[2][:-1, :-1, :3], (seq[2]["indirect"][..., :3] * seq[2]["albedo"][..., :3])[:-1, :-1])  # history was in use


@pytest.mark.parametrize("w,h", [(1, 1), (9, 3), (33, 9), (7, 130)])
def test_tiled_path_equals_gathered_in_fast_mode(native_lib, bluenoise, w, h):
    """test_post_planes_gpu.py::test_tiled_path_at_sizes_with_sky's scenes with both entry points in fast mode: cap_post_frame (the
    only way to the TILED fast Gather, k_stencil_lds<kGather, ..., FAST, TILED>, and to Combine on tiled direct and albedo) and
    cap_post_frame_gathered with one shard on the resolved tiles agree bit for bit -- stage_texel<TILED> untiles and decodes with
    k_untile_decode's operations, so the same bits; the rendered-frame tolerance cannot see an error below its 3 %."""
    arrays = quad_scene(w, h)
    r = capi.Renderer(0)
    r.upload_scene(*arrays)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    r.set_resolution(w, h)
    cams = [quad_camera(w, h, 0.01 * k) for k in range(4)]
    gs = capi.PostSettings(fast_weights=1)

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

    tiled, gathered = sequence(False), sequence(True)
    r.close()
    assert all(np.all(np.isfinite(o)) for o in tiled)
    assert_same_bits(tiled, gathered, "fast cap_post_frame against cap_post_frame_gathered(1) %dx%d" % (w, h))
