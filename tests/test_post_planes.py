"""CPU side of the crafted-plane cases of the reconstruction chain (tests/post_planes_support.py): every case that is named after a
path of post.hip proves with the restated predicates that its planes reach that path, the oracle's output is finite on all of them,
sky pixels pass through in closed form, and the tiling helper the device side uploads through is the inverse of its assembly.
Also the conditions on the reference alone that the fast mode's bound rests on (S.sensitivity; tests/test_post_planes_fast_gpu.py):
which frames are too ill-conditioned for their maximum to be judged, that every judged sensitivity is finite and non-zero, and
that the perturbed draws take the exact run's decisions."""
import numpy as np
import pytest

import post_planes_support as S
from capsaicin_amd import tiles
from oracle import cap_oracle as O

F = np.float32
ALL_SIZES = S.SIZES + S.SIZES_LOWRES + [(S.BW, S.BH), (S.SW, S.SH), (7, 130)]


def depth_of(frame):
    return frame[3]["normal_depth"][..., 3]


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_oracle_is_finite_and_inputs_keep_the_value_contract(name):
    c = S.CASES[name]()
    assert len(c.frames) >= S.N_FRAMES
    for _, _, _, p in c.frames:
        for k in ("indirect", "direct", "albedo"):
            assert np.all(np.isfinite(p[k])) and p[k].min() >= 0.0 and p[k].max() <= 1e30
        assert np.all(np.isfinite(p["normal_depth"])) and p["normal_depth"][..., 3].min() >= 0.0
    for f, out in enumerate(S.oracle_outputs(name)):
        assert out.shape == (c.h, c.w, 4) and np.all(np.isfinite(out)), f


@pytest.mark.parametrize("name", sorted(n for n in S.CASES if "lowres" not in n))
def test_sky_pixels_pass_through(name):
    """As test_oracle_post.test_sky_pixels_pass_through, on every case with sky texels: the output there is
    min(indirect, 10) * albedo + direct bit for bit (output 1: direct, 2: min(indirect, 10), 3: the variance Accumulate left, 0;
    without the denoiser nothing clamps).  Checked where the pixel centre survives the UV round trip (at 40 x 24 that is every pixel
    but the last row and column, the other test's exclusion); the half-resolution chain resamples its colour and is left out."""
    c = S.CASES[name]()
    s = O.PostSettings(**c.settings)
    assert not s.lowres_indirect
    exact = S.centre_survives_uv(c.w, c.h)
    outs = S.oracle_outputs(name)
    for (f, _, _, p), out in zip(c.frames, outs):
        sky = S.is_background(p["normal_depth"][..., 3]) & exact
        ind = S.remove_fireflies(p["indirect"][..., :3]) if s.denoise else p["indirect"][..., :3]
        want = {0: ind * p["albedo"][..., :3] + p["direct"][..., :3], 1: p["direct"][..., :3], 2: ind, 3: np.zeros_like(ind)}[s.output]
        assert np.array_equal(S.bits(out[..., :3])[sky], S.bits(want.astype(F))[sky]), (name, f)
        assert np.all(out[..., 3] == 1.0)
    if "sky" in c.info:
        assert sky.sum() > 0.2 * S.sky_pattern(c.info["sky"]).sum()  # the check is not vacuous


def test_centre_survives_uv_is_the_other_tests_exclusion():
    m = S.centre_survives_uv(40, 24)
    assert m[:-1, :-1].all() and not m[-1].any() and not m[:, -1].any()


@pytest.mark.parametrize("w,h", ALL_SIZES)
def test_tiling_helper_round_trip(w, h):
    img = np.random.default_rng(w * 1000 + h).random((h, w, 4)).astype(F)
    buf = tiles.extract(img, 0, 1)
    assert buf.shape == (tiles.padded_pixels(w, h, 1), 4)
    assert np.array_equal(tiles.assemble([buf], w, h), img)


def test_tile_geometry_restatements_partition_the_image():
    """Every pixel is the own pixel of exactly one stencil tile and, per stride, of exactly one phase tile."""
    for w, h in ALL_SIZES:
        tx, ty = S.stencil_tiles(w, h)
        n = sum(S.stencil_tile(w, h, bx, by, 3)[0].astype(int) for by in range(ty) for bx in range(tx))
        assert np.all(n == 1), (w, h)
        for stride in (3, 5, 7):
            n = sum(S.phase_tile(w, h, stride, *t)[0].astype(int) for t in S.all_phase_tiles(w, h, stride))
            assert np.all(n == 1), (w, h, stride)


def test_sizes_reach_unequal_row_phases_and_nearly_empty_tiles():
    """What the size list is there for: less than a workgroup, exact fits, one over; heights whose stride-3/5/7 row phases hold
    unequal row counts; last phase tiles of one column and two or three rows."""
    assert (32, 8) in S.SIZES and (33, 9) in S.SIZES and (31, 7) in S.SIZES and (64, 8) in S.SIZES and (65, 17) in S.SIZES
    for h in (17, 23, 57):
        for stride in (3, 5, 7) if h != 57 else (5, 7):  # (57 = 3 * 19)
            rows = [len(range(py, h, stride)) for py in range(stride)]
            assert min(rows) != max(rows), (h, stride)
    w, h = 129, 57  # stride 3: 19 rows per phase = two full 8-row tiles and one of three rows; the third 64-column tile holds one column
    rows = sorted(int(S.phase_tile(w, h, 3, t[0], t[1], t[2])[0].sum()) for t in S.all_phase_tiles(w, h, 3))
    assert rows[0] == 3 and rows[-1] == 64 * 8
    assert min(int(S.phase_tile(65, 17, 7, *t)[0].sum()) for t in S.all_phase_tiles(65, 17, 7)) == 2  # one column, two rows


@pytest.mark.parametrize("kind", S.SKY_KINDS)
def test_reach_sky_taps_are_kept_out_by_the_background_select_alone(kind):
    """A sky texel's cleared normal decodes to (0, 0, -1).  Against walls that face the camera its normal weight would be 0 with or
    without the select on the tap's depth (post.hip:704, 822); the sky cases' walls face away, so the normal weight of a sky tap is
    close to 1, its depth weight exp(-1 / (sigma len)) -- and sky and geometry are neighbours."""
    c = S.CASES["e-sky-%s-out0" % kind]()
    nd = c.frames[0][3]["normal_depth"]
    sky = S.is_background(nd[..., 3])
    assert np.array_equal(sky, S.sky_pattern(kind))
    sky_normal = S.oct_decode(np.zeros(2, F))
    assert np.allclose(sky_normal, (0, 0, -1))
    if kind == "all":
        return
    assert (S.oct_decode(nd[..., 0:2])[~sky] @ sky_normal).min() > 0.99
    assert (sky[:, 1:] != sky[:, :-1]).any() and (sky[1:] != sky[:-1]).any()


def staged_luma_in_range(c):
    """Every colour a stencil pass can stage -- the raw indirect image (Gather) and Accumulate's clamped output (the others start
    from it) -- has a luminance inside div_unscaled's range, so depth alone decides the form."""
    ok = True
    for (_, _, _, p), (col, _) in zip(c.frames, S.trace_accumulate(c.w, c.h, c.settings, c.frames)):
        ok &= bool(S.div_luma_ok(S.luminance(p["indirect"])).all()) and bool(S.div_luma_ok(S.luminance(S.remove_fireflies(col[..., :3]))).all())
    return ok


@pytest.mark.parametrize("name", ["b-halo-left", "b-halo-above", "b-halo-corner"])
def test_reach_far_texel_lies_in_a_halo_only(name):
    c = S.CASES[name]()
    x, y = c.info["texel"]
    bx, by = c.info["tile"]
    assert staged_luma_in_range(c)
    for fr in c.frames:
        d = depth_of(fr)
        bad = ~S.div_depth_ok(d)
        assert bad.sum() == 1 and bad[y, x] and d[y, x] > 2.0 ** 40
        for R in (3, 2):  # Gather / BlurDisocclusion, the first a-trous pass
            own, staged = S.stencil_tile(c.w, c.h, bx, by, R)
            assert own.sum() == 32 * 8 and not (bad & own).any() and (bad & staged).sum() == 1
        for stride in (3, 5, 7):
            halo_only = [t for t in S.all_phase_tiles(c.w, c.h, stride)
                         if (lambda o, s: bool(s[y, x]) and not o[y, x])(*S.phase_tile(c.w, c.h, stride, *t))]
            stages = [t for t in S.all_phase_tiles(c.w, c.h, stride) if S.phase_tile(c.w, c.h, stride, *t)[1][y, x]]
            assert stages  # some phase tile fails its range test on this one texel
            if name != "b-halo-above":  # (at 24 rows a phase is a single tile: the row halo holds no other tile's pixels)
                assert halo_only, stride


def test_reach_one_lane_outside_its_tile_inside():
    c = S.CASES["c-one-lane"]()
    x, y = c.info["pixel"]
    assert staged_luma_in_range(c)
    sd = F(c.settings["eaw_depth_sigma"])
    assert sd == F(c.settings["gather_depth_sigma"]) == F(3.0)
    for fr in c.frames:
        d = depth_of(fr)
        assert S.div_depth_ok(d).all() and not S.is_background(d).any()  # every tile's range test holds
        assert d[y, x] == F(2.0 ** 39)
        for stride in (1, 3, 5, 7):  # k.s_depth = cd * sigma (post.hip:679) and cd * stride * sigma (:802)
            bad = ~S.div_sigma_ok(d * F(stride) * sd)
            assert bad.sum() == 1 and bad[y, x]
            assert d[y, x] * F(stride) * sd > F(2.0 ** 38)


def test_reach_luminance_below_the_range():
    c = S.CASES["d-luma-tiny"]()
    # 3 pixels of Gather's 7 x 7, one of Accumulate's bilinear tap (where the pixel centre does not survive the UV round trip it
    # blends a neighbour in with weight 1 - 2^-24, which leaves 2^-25 of an ordinary value) and one of the bicubic history resample
    inner = (slice(S.BLOCK[0].start + 5, S.BLOCK[0].stop - 5), slice(S.BLOCK[1].start + 5, S.BLOCK[1].stop - 5))
    assert S.BLOCK[0].stop - S.BLOCK[0].start >= 15 and S.BLOCK[1].stop - S.BLOCK[1].start >= 15
    for f, (col, _) in enumerate(S.trace_accumulate(c.w, c.h, c.settings, c.frames)):
        lum = S.luminance(S.remove_fireflies(col[..., :3]))[inner]
        assert np.all(lum > 0) and np.all(lum < F(2.0 ** -50)) and not S.div_luma_ok(lum).any(), f
        outside = np.ones((c.h, c.w), bool)
        outside[S.BLOCK] = False
        assert S.div_luma_ok(S.luminance(col[..., :3]))[outside].mean() > 0.9  # an image of ordinary values around it


def test_reach_luminance_at_the_firefly_clamp():
    c = S.CASES["d-luma-clamp"]()
    inner = (slice(S.BLOCK[0].start + 3, S.BLOCK[0].stop - 3), slice(S.BLOCK[1].start + 3, S.BLOCK[1].stop - 3))
    for f, (col, _) in enumerate(S.trace_accumulate(c.w, c.h, c.settings, c.frames)):
        lum = S.luminance(col[..., :3])
        assert lum[4:20, 56:60].min() > 1e3, f  # far above the clamp after Gather and Accumulate
        assert S.luminance(S.remove_fireflies(col[..., :3]))[4:20, 56:60].max() <= F(10.0) * (1 + 2 ** -22)
        assert np.all(lum[inner] > 9.9) and np.all(lum[inner] <= F(10.0)), f


def test_reach_luminance_exactly_zero():
    c = S.CASES["d-luma-zero-tile"]()
    own, _ = S.stencil_tile(c.w, c.h, *c.info["tile"], 3)
    for f, ((_, _, _, p), (col, _)) in enumerate(zip(c.frames, S.trace_accumulate(c.w, c.h, c.settings, c.frames))):
        assert np.all(p["indirect"][own][:, :3] == 0.0)
        lum = S.luminance(col[..., :3])
        assert np.all(lum[11:13, 36:60] == 0.0), f  # rows whose 7 x 7 Gather footprint lies inside the tile
        assert (lum[own] > 0).any()  # and the tile's rim blends with its neighbours: zero and non-zero luminances in one tile


def test_reach_sparse_disocclusion_and_dual_read():
    c = S.CASES["f-sparse-disocclusion"]()
    tr = S.trace_accumulate(c.w, c.h, c.settings, c.frames)
    hist = [m[..., 3] for _, m in tr]
    patch = np.zeros((c.h, c.w), bool)
    patch[S.PATCH] = True
    assert np.all(hist[6] == 7.0)
    for f in range(7, S.PATCH_FRAME):
        assert np.all(hist[f] >= 8.0), f  # every workgroup of BlurDisocclusion returns early (post.hip:638-645)
    at = hist[S.PATCH_FRAME]
    assert np.all(at[~patch] >= 8.0) and np.all(at[patch] < 8.0)
    bx, by = c.info["tile"]
    own, _ = S.stencil_tile(c.w, c.h, bx, by, 3)
    assert patch[own].sum() == patch.sum()  # the patch lies in one tile: only that workgroup runs its taps again
    for nb in ((bx - 1, by), (bx, by - 1), (bx - 1, by - 1)):  # its neighbours return early, and the first a-trous pass
        nown, nstaged = S.stencil_tile(c.w, c.h, nb[0], nb[1], 2)  # stages the patch from BlurDisocclusion's image in their halo
        assert np.all(at[nown] >= 8.0) and (patch & nstaged).any() and not (patch & nown).any()
    assert len(c.frames) > S.PATCH_FRAME + 2 and (hist[S.PATCH_FRAME + 1] < 8.0).sum() > patch.sum()  # then the patch's rim resets too


# ---- the two cases the fast accumulate needs -----------------------------------------------------------------------------------------
def test_reach_reprojection_into_the_outermost_ring():
    """h-reproject-ring: in some frame a non-sky pixel reprojects (a) into the outermost texel ring, where the 3 x 3 of previous
    depths has taps outside the image, and (b) onto a previous-frame sky texel that has geometry among its in-image neighbours --
    closest_depth's start from a centre of 0.  Counted with the float64 restatements of the known-answer tests."""
    import test_oracle_post_kat as K
    c = S.CASES["h-reproject-ring"]()
    w, h = c.w, c.h
    ring = S.sky_ring(w, h)
    frames_a, frames_b = 0, 0
    for f in range(1, len(c.frames)):
        _, cam, prev, p = c.frames[f]
        nd, prev_nd = p["normal_depth"], c.frames[f - 1][3]["normal_depth"]
        assert np.array_equal(S.is_background(nd[..., 3]), ring)
        n_a = n_b = 0
        for y, x in np.argwhere(~ring & ~S._box(w, h, 4, w - 4, 4, h - 4)):  # (only pixels near the border can land in the ring)
            uv = (np.array([x, y], np.float64) + 0.5) / np.array([w, h], np.float64)
            puv = K.image_plane_uv(prev, K.reconstruct_world_position(cam, uv, float(nd[y, x, 3])))
            if puv[0] < 0 or puv[1] < 0 or puv[0] > 1 or puv[1] > 1:
                continue
            cx, cy = (int(v) for v in K.uv_to_xy(puv, w, h))
            if not ring[cy, cx]:
                continue
            n_a += 1
            around = prev_nd[max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2, 3]
            n_b += int(prev_nd[cy, cx, 3] == 0.0 and (around != 0.0).any() and K.closest_depth(prev_nd, (cx, cy)) == 0.0)
        frames_a += n_a > 0
        frames_b += n_b > 0
    assert frames_a >= 1 and frames_b >= 1
    assert frames_a >= 6  # (as built: the yaw carries a column of pixels into the ring in every frame)


def test_reach_constant_planes():
    c = S.CASES["h-constant"]()
    assert len({bytes(fr[1]) for fr in c.frames}) == len(c.frames)  # the camera turns every frame
    assert bytes(c.frames[6][2]) != bytes(c.frames[5][1])  # and frame 6 reprojects through the cut
    for _, _, _, p in c.frames:
        assert np.all(p["indirect"][..., :3] == F(S.CONSTANT_VALUE)) and np.all(p["albedo"][..., :3] == 1.0) and np.all(p["direct"][..., :3] == 0.0)
        assert not S.is_background(p["normal_depth"][..., 3]).any() and len(np.unique(S.second_wall_mask(c.w, c.h))) == 2
    # the exact output is the constant within the fixed-point test's bound (tests/test_oracle_post.py), and the chain's answer to
    # a relative input change of delta is of delta's order in the median once the zero history of frame 0 has decayed (that frame's
    # TAA clip box is rounding noise wide, see the fixed-point test)
    for out in S.oracle_outputs("h-constant"):
        assert np.abs(out[..., :3] - S.CONSTANT_VALUE).max() < 5e-3
    assert S.PERTURBATION / 8 < S.sensitivity("h-constant")[:, 0].min() < 2 * S.PERTURBATION


# ---- conditions on the reference alone that the fast mode's bound rests on (tests/test_post_planes_fast_gpu.py) ------------------------
def test_ill_conditioned_frames_are_the_stated_ones():
    """A frame whose own Smax exceeds 3e-2 answers a 2^-16 input change with more than the header's largest stated error: its
    maximum is not judged.  That happens in the late frames of d-luma-clamp only (1e6 fireflies beside a block at the clamp)."""
    ill = [(n, f) for n in sorted(S.CASES) for f, s in enumerate(S.sensitivity(n)) if s[2] > S.ILL_CONDITIONED]
    assert sum(len(S.CASES[n]().frames) for n in S.CASES) == 662 + 2 * S.N_FRAMES
    assert {n for n, _ in ill} == {"d-luma-clamp"} and len(ill) <= 6, ill
    assert all(f >= 7 for _, f in ill), ill


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_sensitivity_is_finite_and_non_zero_where_it_is_judged(name):
    """A zero S would leave the 2^-20 floor as the whole budget, an infinite one no bound at all.  All three colour planes are
    perturbed for this: with the indirect plane alone output = 1 (the direct term) would not move.  Zero remains where the exact
    output is identically 0 -- the variance image of an all-sky frame."""
    c = S.CASES[name]()
    s = S.sensitivity(name)
    assert s.shape == (len(c.frames), 3) and np.all(np.isfinite(s)) and np.all(s[:, 0] <= s[:, 1]) and np.all(s[:, 1] <= s[:, 2])
    if c.w * c.h < S.SMALL_IMAGE:
        assert s[:, 2].max() > 0.0
        return
    for f, out in enumerate(S.oracle_outputs(name)):
        if np.all(out[..., :3] == 0.0):
            assert name == "e-sky-all-out3" and np.all(s[f] == 0.0)
        else:
            assert np.all(s[f] > 0.0), (f, s[f])


@pytest.mark.parametrize("name", ["g-camera-yaw", "f-sparse-disocclusion", "h-reproject-ring"])
def test_perturbed_draws_take_the_exact_runs_decisions(name):
    """normal_depth and the cameras are not perturbed, so reset, reprojection and history length -- what Accumulate DECIDES, and what
    BlurDisocclusion's pass-through reads -- are the unperturbed sequence's in every frame."""
    c = S.CASES[name]()
    exact = S.trace_accumulate(c.w, c.h, c.settings, c.frames)
    seen = set()
    for draw in (0, S.DRAWS - 1):
        pert = S.trace_accumulate(c.w, c.h, c.settings, S.perturbed_frames(name, draw))
        for (col, mom), (pcol, pmom) in zip(exact, pert):
            assert np.array_equal(mom[..., 3], pmom[..., 3])
            assert not np.array_equal(col[..., :3], pcol[..., :3])  # (the colours did move)
            seen |= set(np.unique(mom[..., 3]).tolist())
    assert 1.0 in seen and max(seen) >= 8.0  # resets and long histories both occur
