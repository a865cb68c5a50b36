"""Crafted input planes for the reconstruction chain (post.hip) and the two sides they run on.

The chain's result depends on decisions a pixel, a wave or a workgroup takes on its own: the division form (div_unscaled or the IEEE
division, per tile while staging and again per wave), BlurDisocclusion's early return and the DUAL read behind it, zero-weight taps on
background and out-of-image texels, the 32 x 8 / 64 x 8-row-phase tile geometry, and the reprojection footprints at the image border.
Rendered Cornell frames reach few of them, so the sequences here are built by hand: cap_post_frame_gathered with shard_count 1 takes
four caller-made planes in tile order (tiles.extract(image, 0, 1)), O.PostChain.frame the same planes row-major.

  run_gpu / run_oracle     one sequence of frames on the device / through the oracle's chain
  CASES                    name -> builder of a `Case` (size, settings, frames, and what its reach check needs)
  div_*_ok, is_background, stencil_tile, phase_tile
                           numpy restatements of post.hip's decision predicates, so that a CPU test can prove that a case reaches
                           the path it is named after (tests/test_post_planes.py)
  trace_accumulate         Gather and Accumulate alone (O.post_pass) with their histories carried: the images the later passes stage

The renderer needs a resolution and a camera for this entry point, no scene.  Value contract of everything built here: colours
finite, non-negative and at most 1e30; depths finite and non-negative (0 = sky).

`fast_weights` (the toleranced mode, not an option of the oracle) runs on the same cases: run_gpu takes it as a key of the settings,
run_oracle drops it, and `sensitivity` gives the bound it is held to (tests/test_post_planes_fast_gpu.py): what the oracle's exact
chain itself answers to a 2^-16 relative change of its colour inputs."""
import functools

import numpy as np

from oracle import cap_oracle as O
from test_oracle_post import wall_planes

PLANE_ORDER = ("indirect", "direct", "albedo", "normal_depth")  # the chain's order (ctx_post.hip cap_resolve_aov_tiles)
N_FRAMES = 12  # history lengths pass 8 (BlurDisocclusion's pass-through, post.hip:638)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- cameras -------------------------------------------------------------------------------------------------------------------
def make_cam(w, h, pos=(0.0, 0.0, 0.0), yaw=0.0, focal=0.035, back=False):
    """The camera of test_oracle_post.camera turned by `yaw` about +y (back: facing +z instead of -z); right and up by the
    reference's formulas (input_system.cpp:134-141), as capi.camera_from_config forms them."""
    f = np.float64([np.sin(yaw), 0.0, -np.cos(yaw)]) * (-1.0 if back else 1.0)
    right = -np.cross(f, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    up = np.cross(f, right)
    return O.make_camera(tuple(pos), tuple(f), tuple(right), tuple(up), 0.036, 0.036 * h / w, focal)


def capi_cam(cam):
    from capsaicin_amd import capi
    return capi.CameraData.from_buffer_copy(bytes(cam))  # the same 72-byte CameraData layout on both sides


def oracle_cam(cam):
    return O.Camera.from_buffer_copy(bytes(cam))


# ---- plane builders --------------------------------------------------------------------------------------------------------------
SECOND_WALL_NORMAL = (0.05, 0.02, 1.0)  # n . (0, 0, 1) = 0.9986: a normal weight of 0.83 (sigma 128) / 0.91 (sigma 64), not 0 or 1
SECOND_WALL_DEPTH = 1.5                 # depth ratio of the second wall (z = -3): a depth weight of exp(-1 / (6 len)) at the seam


def second_wall_mask(w, h):
    """The lower right of a diagonal seam, so that the seam crosses tile boundaries in both directions."""
    ys, xs = np.mgrid[0:h, 0:w]
    return (2 * xs + 3 * ys) >= (w + 1.5 * h)


def two_walls(w, h, cam, rng=None, value=0.5, flip=False):
    """wall_planes plus a second wall at another depth with another normal, a direct term and a varying albedo.
    flip: both normals point away from the camera (z < 0).  A sky texel's cleared normal (0, 0) decodes to (0, 0, -1), so against
    walls that face the camera its normal weight is 0 whatever the background select does (post.hip:704, 822); against flipped walls
    it is ~1 and only the select keeps the tap out of the sums."""
    p = wall_planes(w, h, cam, rng=rng, value=value)
    m = second_wall_mask(w, h)
    n = np.float32(SECOND_WALL_NORMAL)
    n /= np.linalg.norm(n)
    if flip:
        n[2] = -n[2]
        p["normal_depth"][..., 0:2] = O.oct_encode(np.float32([0.0, 0.0, -1.0]))
    p["normal_depth"][m, 0:2] = O.oct_encode(n)
    p["normal_depth"][m, 3] *= np.float32(SECOND_WALL_DEPTH)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    p["albedo"][..., 0] = 0.25 + 0.5 * ((xs * 7 + ys * 3) % 11) / 11
    p["albedo"][..., 1] = 0.9
    p["albedo"][..., 2] = 0.4 + 0.05 * (ys % 5)
    p["direct"][..., 0:3] = (0.125 * ((xs + 2 * ys) % 4))[..., None]
    p["direct"][..., 3] = 1.0
    return p


def punch_sky(planes, mask):
    """Sky texels: the G-buffer's cleared value, normal_depth = 0 (depth < 1e-5 is the background test of every pass)."""
    planes["normal_depth"][mask] = 0.0
    return planes


def few_sky(w, h, seed=99):
    m = np.random.default_rng(seed).random((h, w)) < 0.04
    m[0, 0] = False
    return m


class Case:
    def __init__(self, w, h, frames, settings=None, **info):
        self.w, self.h, self.frames, self.settings, self.info = w, h, frames, dict(settings or {}), info


def static_frames(w, h, make_planes, n=N_FRAMES, cams=None, prevs=None):
    """frames[f] = (frame_count, cam, prev_cam, planes); make_planes(f, cam) builds frame f's planes; prevs overrides single
    previous cameras ({frame: cam})."""
    cams = cams or [make_cam(w, h)] * n
    out = []
    for f in range(n):
        prev = cams[max(f - 1, 0)]
        if prevs and f in prevs:
            prev = prevs[f]
        out.append((f, cams[f], prev, make_planes(f, cams[f])))
    return out


def noisy_two_walls(w, h, seed, sky=None, edit=None, flip=False):
    """make_planes for static_frames: two walls with fresh noise every frame (fixed seed), sky mask, then `edit(f, planes)`."""
    rng = np.random.default_rng(seed)

    def make(f, cam):
        p = two_walls(w, h, cam, rng=rng, flip=flip)
        if sky is not None:
            punch_sky(p, sky)
        if edit:
            edit(f, p)
        return p
    return make


# ---- the two sides ---------------------------------------------------------------------------------------------------------------
def lowres_offset(frame_count):
    return (frame_count % 4) // 2, (frame_count % 4) % 2  # (ox, oy), rt_indirect.hlsl:53-59


def oracle_settings(settings):
    """O.PostSettings of a case's settings: `fast_weights` is the device's switch alone and has no field there."""
    return O.PostSettings(**{k: v for k, v in dict(settings).items() if k != "fast_weights"})


def run_oracle(w, h, settings, frames):
    s = oracle_settings(settings)
    chain = O.PostChain(w, h)
    out = []
    for fc, cam, prev, planes in frames:
        if s.lowres_indirect:
            ox, oy = lowres_offset(fc)
            planes = dict(planes, indirect_lowres=planes["indirect"][oy::2, ox::2])  # what cap_post_frame_gathered decimates
        out.append(chain.frame(s, fc, cam, prev, planes))
    return out


def run_gpu(r, settings, frames):
    """`r`: a capi.Renderer with its resolution set (unsharded).  One upload, one cap_post_frame_gathered, one readback per frame.
    settings may hold fast_weights = 1: the toleranced mode."""
    import torch
    from capsaicin_amd import capi, tiles
    s = capi.PostSettings(**settings)
    out = []
    for fc, cam, prev, planes in frames:
        r.set_camera(capi_cam(cam))
        tiled = np.concatenate([tiles.extract(np.ascontiguousarray(planes[k], np.float32), 0, 1) for k in PLANE_ORDER])
        t = torch.from_numpy(np.ascontiguousarray(tiled, np.float32).ravel()).to("cuda")
        assert t.numel() == r.aov_tile_buffer_floats()
        torch.cuda.synchronize()  # the renderer runs on its own stream
        r.post_frame_gathered(s, fc, capi_cam(prev), t.data_ptr(), 1)
        out.append(r.post_readback())  # (synchronises: `t` outlives the chain's reads)
    return out


def trace_accumulate(w, h, settings, frames):
    """Gather -> Accumulate alone, histories carried as oracle_post_frame carries them (full-resolution form).
    -> per frame (accumulated colour | variance, moments | history length)."""
    s = oracle_settings(settings)
    assert not s.lowres_indirect
    z = np.zeros((h, w, 4), np.float32)
    chist, mhist, prev_nd, out = z, z, z, []
    for fc, cam, prev, planes in frames:
        col = planes["indirect"]
        if s.gather:
            col, _ = O.post_pass(0, s, [col, planes["normal_depth"]])
        chist, mhist = O.post_pass(1, s, [col, planes["normal_depth"], chist, mhist, prev_nd], arg=fc, cam=cam, prev_cam=prev)
        prev_nd = planes["normal_depth"]
        out.append((chist, mhist))
    return out


# ---- post.hip's decision predicates, restated --------------------------------------------------------------------------------------
F = np.float32


def div_sigma_ok(s):  # post.hip:137
    s = np.asarray(s, F)
    return (s == 0) | ((s >= F(2.0 ** -38)) & (s <= F(2.0 ** 38)))


def div_depth_ok(d):  # post.hip:136, 138
    d = np.asarray(d, F)
    return (d < F(1e-5)) | (d <= F(2.0 ** 40))


def div_luma_ok(l):  # post.hip:139
    l = np.asarray(l, F)
    return (l == 0) | ((l >= F(2.0 ** -50)) & (l <= F(2.0 ** 30)))


def is_background(d):  # post.hip:285, 590, 638, 704, 798: depth < 1e-5
    return np.asarray(d, F) < F(1e-5)


def luminance(c):  # post.hip:46
    c = np.asarray(c, F)
    return c[..., 0] * F(0.299) + c[..., 1] * F(0.587) + c[..., 2] * F(0.114)


def oct_decode(xy):  # post.hip:112-120
    f = np.asarray(xy, F) * F(2.0) - F(1.0)
    n = np.stack([f[..., 0], f[..., 1], F(1.0) - np.abs(f[..., 0]) - np.abs(f[..., 1])], -1)
    t = np.clip(-n[..., 2], F(0.0), F(1.0))
    n[..., 0] += np.where(n[..., 0] >= 0, -t, t)
    n[..., 1] += np.where(n[..., 1] >= 0, -t, t)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def remove_fireflies(c):  # post.hip:464, 591
    return np.minimum(np.asarray(c, F), F(10.0))


def _box(w, h, x0, x1, y0, y1):
    m = np.zeros((h, w), bool)
    m[max(y0, 0):max(min(y1, h), 0), max(x0, 0):max(min(x1, w), 0)] = True
    return m


def stencil_tiles(w, h):  # post.hip:614
    return (w + 31) // 32, (h + 7) // 8


def stencil_tile(w, h, bx, by, R):
    """(own, staged) pixel masks of workgroup tile (bx, by) of k_stencil_lds: 32 x 8 pixels, staged with a halo of R on every side
    (post.hip:609, 615-616, 655; R = 3 for Gather and BlurDisocclusion, 2 for the first a-trous pass).  Texels outside the image
    are staged as zeros, which pass both range tests, so the masks are clipped to the image."""
    return _box(w, h, bx * 32, bx * 32 + 32, by * 8, by * 8 + 8), _box(w, h, bx * 32 - R, bx * 32 + 32 + R, by * 8 - R, by * 8 + 8 + R)


def phase_tiles(w, h, stride):  # post.hip:753, 1152: (tiles_x, tiles_per_phase); the grid holds tiles_x * tiles_per_phase * stride tiles
    return (w + 63) // 64, ((h + stride - 1) // stride + 7) // 8


def phase_tile(w, h, stride, tx, jt, py):
    """(own, staged) masks of k_blur_phase's tile: 64 columns with a halo of 2 * stride, rows py + stride * j for j in
    [8 jt, 8 jt + 8) with two more such rows on either side (post.hip:758, 764-765, 776, 787)."""
    own, staged = np.zeros((h, w), bool), np.zeros((h, w), bool)
    for j in range(jt * 8 - 2, jt * 8 + 10):
        y = py + stride * j
        if 0 <= y < h:
            staged[y] = _box(w, 1, tx * 64 - 2 * stride, tx * 64 + 64 + 2 * stride, 0, 1)[0]
            if jt * 8 <= j < jt * 8 + 8:
                own[y] = _box(w, 1, tx * 64, tx * 64 + 64, 0, 1)[0]
    return own, staged


def all_phase_tiles(w, h, stride):
    ptx, ptp = phase_tiles(w, h, stride)
    return [(tx, jt, py) for py in range(stride) for jt in range(ptp) for tx in range(ptx)]


def centre_survives_uv(w, h):
    """Pixels whose centre survives the reference's UV round trip exactly, ((x + 0.5) / w) * w == x + 0.5 in float32 (utils.h:6-16):
    there SampleBilinear's fractional weights are exactly 0 and the tap is the texel.  The last row and column never do (UVtoXY
    clamps to dim - 1)."""
    def ok(n):
        c = np.arange(n, dtype=F) + F(0.5)
        return ((c / F(n)) * F(n) == c) & (np.arange(n) < n - 1)
    return ok(h)[:, None] & ok(w)[None, :]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (2, 2), (5, 1), (1, 9), (31, 7), (32, 8), (33, 9), (64, 8), (65, 17), (70, 23), (129, 57)]
SIZES_SETTINGS = [(33, 9), (65, 17), (70, 23)]
SIZES_LOWRES = [(2, 2), (34, 10), (66, 58)]
CASES = {}


def case(name):
    def reg(fn):
        CASES[name] = functools.lru_cache(maxsize=None)(fn)
        return fn
    return reg


def _sizes_case(w, h, settings):
    return Case(w, h, static_frames(w, h, noisy_two_walls(w, h, 1000 + 31 * w + h, sky=few_sky(w, h))), settings)


for _w, _h in SIZES:
    case("a-size-%dx%d" % (_w, _h))(functools.partial(_sizes_case, _w, _h, ()))
for _w, _h in SIZES_SETTINGS:
    # (gather = 0: the gathered entry point's plain copy of the indirect plane, which no rendered-frame test takes)
    for _name, _s in (("eaw3", (("eaw5", 0),)), ("novar", (("use_variance", 0),)), ("nodenoise", (("denoise", 0),)), ("nogather", (("gather", 0),))):
        case("a-%s-%dx%d" % (_name, _w, _h))(functools.partial(_sizes_case, _w, _h, _s))
for _w, _h in SIZES_LOWRES:
    case("a-lowres-%dx%d" % (_w, _h))(functools.partial(_sizes_case, _w, _h, (("lowres_indirect", 1),)))

BW, BH = 96, 24  # 3 x 3 stencil tiles, 2 phase-tile columns
FAR_DEPTH = 3e12  # above 2^40 = 1.1e12


def _far_texel_case(x, y, tile):
    def edit(f, p):
        p["normal_depth"][y, x, 3] = FAR_DEPTH
    return Case(BW, BH, static_frames(BW, BH, noisy_two_walls(BW, BH, 7 + x + y, edit=edit)), texel=(x, y), tile=tile)


# the texel lies in the halo of stencil tile (2, 1) = pixels [64, 96) x [8, 16) and in none of its pixels
case("b-halo-left")(functools.partial(_far_texel_case, 63, 12, (2, 1)))
case("b-halo-above")(functools.partial(_far_texel_case, 72, 7, (2, 1)))
case("b-halo-corner")(functools.partial(_far_texel_case, 63, 7, (2, 1)))


@case("c-one-lane")
def _one_lane():
    x, y = 40, 12

    def edit(f, p):
        p["normal_depth"][y, x, 3] = 2.0 ** 39
    return Case(BW, BH, static_frames(BW, BH, noisy_two_walls(BW, BH, 21, edit=edit)),
                dict(eaw_depth_sigma=3.0, gather_depth_sigma=3.0), pixel=(x, y))


BLOCK = (slice(4, 20), slice(40, 56))  # 16 x 16 pixels: rows 4..19, columns 40..55 (across stencil tiles and both phase columns)


@case("d-luma-tiny")
def _luma_tiny():
    def edit(f, p):
        p["indirect"][BLOCK + (slice(0, 3),)] = 1e-20
    return Case(BW, BH, static_frames(BW, BH, noisy_two_walls(BW, BH, 31, edit=edit)))


@case("d-luma-clamp")
def _luma_clamp():
    def edit(f, p):
        p["indirect"][BLOCK + (slice(0, 3),)] = 9.99
        p["indirect"][4:20, 56:60, 0:3] = 1e6  # fireflies beside the block: clamped to 10 by every pass but Gather
    return Case(BW, BH, static_frames(BW, BH, noisy_two_walls(BW, BH, 32, edit=edit)))


@case("d-luma-zero-tile")
def _luma_zero():
    def edit(f, p):
        p["indirect"][8:16, 32:64, 0:3] = 0.0  # stencil tile (1, 1)
    return Case(BW, BH, static_frames(BW, BH, noisy_two_walls(BW, BH, 33, edit=edit)), tile=(1, 1))


SW, SH = 70, 23


def sky_pattern(kind, w=SW, h=SH):
    ys, xs = np.mgrid[0:h, 0:w]
    if kind == "checker":
        return (xs + ys) % 2 == 0
    if kind == "cross":  # a row and a column crossing the 32 x 8 and 64-column boundaries
        return (ys == 8) | (xs == 33)
    if kind == "frame":
        return (xs < 2) | (ys < 2) | (xs >= w - 2) | (ys >= h - 2)
    if kind == "all":
        return np.ones((h, w), bool)
    raise KeyError(kind)


SKY_KINDS = ("checker", "cross", "frame", "all")


def _sky_case(kind, output):
    return Case(SW, SH, static_frames(SW, SH, noisy_two_walls(SW, SH, 41 + output, sky=sky_pattern(kind), flip=True)),
                dict(output=output), sky=kind)


for _k in SKY_KINDS:
    for _o in range(4):
        case("e-sky-%s-out%d" % (_k, _o))(functools.partial(_sky_case, _k, _o))

PATCH = (slice(8, 11), slice(32, 36))  # rows 8..10, columns 32..35: the top left corner of stencil tile (1, 1)
PATCH_FRAME = 10


@case("f-sparse-disocclusion")
def _sparse():
    rng = np.random.default_rng(51)

    def make(f, cam):
        p = wall_planes(BW, BH, cam, rng=rng)  # one wall: no seam that would reset its histories every frame
        if f >= PATCH_FRAME:
            p["normal_depth"][PATCH + (3,)] *= np.float32(0.5)  # the patch moves to half the depth
        return p
    return Case(BW, BH, static_frames(BW, BH, make, n=14), tile=(1, 1))


def _camera_case(kind):
    w, h, n = SW, SH, N_FRAMES
    base = make_cam(w, h)
    cams, prevs = [base] * n, None
    if kind == "yaw":
        cams = [make_cam(w, h, yaw=0.02 * k) for k in range(n)]
    elif kind == "focal":
        cams = [make_cam(w, h, focal=0.035 + 0.001 * max(k - 3, 0)) for k in range(n)]
    elif kind == "dolly":
        cams = [make_cam(w, h, pos=(0.0, 0.0, -0.05 * k)) for k in range(n)]
    elif kind == "cut":  # the previous camera faces away: every reprojection leaves the image
        prevs = {6: O.make_camera((100.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.036, 0.036 * h / w, 0.035)}
    elif kind == "behind":  # in front of both walls (z = -2, -3), facing back at the camera: every point lies behind it
        prevs = {6: make_cam(w, h, pos=(0.0, 0.0, -0.9), back=True)}
    else:
        raise KeyError(kind)
    return Case(w, h, static_frames(w, h, noisy_two_walls(w, h, 61, sky=few_sky(w, h)), cams=cams, prevs=prevs), camera=kind)


CAMERA_KINDS = ("yaw", "focal", "dolly", "cut", "behind")
for _k in CAMERA_KINDS:
    case("g-camera-%s" % _k)(functools.partial(_camera_case, _k))


def sky_ring(w=SW, h=SH):
    """sky_pattern("frame") narrowed to the outermost texel ring."""
    ys, xs = np.mgrid[0:h, 0:w]
    return (xs < 1) | (ys < 1) | (xs >= w - 1) | (ys >= h - 1)


@case("h-reproject-ring")
def _reproject_ring():
    """A yaw and a dolly at once: pixels beside the ring reproject INTO it -- a 3 x 3 of previous depths with taps outside the image,
    around a centre that is a sky texel (closest_depth starts from 0) with geometry next to it."""
    w, h = SW, SH
    cams = [make_cam(w, h, pos=(0.0, 0.0, -0.05 * k), yaw=0.02 * k) for k in range(N_FRAMES)]
    return Case(w, h, static_frames(w, h, noisy_two_walls(w, h, 71, sky=sky_ring(w, h)), cams=cams), camera="yaw+dolly")


CONSTANT_VALUE = 0.37


@case("h-constant")
def _constant():
    """Both walls, one constant indirect colour in every frame, albedo 1, no direct term, no sky; the yaw cameras and the cut.  The
    exact output is that colour up to the chain's rounding, so a tap that reads what it should not -- outside the image, a stale
    halo, the dummy position of a pixel that reprojects nowhere -- stands out by orders of magnitude."""
    w, h = SW, SH
    cams = [make_cam(w, h, yaw=0.02 * k) for k in range(N_FRAMES)]
    prevs = {6: O.make_camera((100.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.036, 0.036 * h / w, 0.035)}

    def make(f, cam):
        p = two_walls(w, h, cam, value=CONSTANT_VALUE)
        p["albedo"][..., 0:3] = 1.0
        p["direct"][..., 0:3] = 0.0
        return p
    return Case(w, h, static_frames(w, h, make, cams=cams, prevs=prevs), camera="yaw+cut")


@functools.lru_cache(maxsize=None)
def oracle_outputs(name):
    """The oracle's frames of a case, computed once and shared (read-only) by the tests that need them."""
    c = CASES[name]()
    out = run_oracle(c.w, c.h, c.settings, c.frames)
    for o in out:
        o.setflags(write=False)
    return out


# ---- the exact chain's own sensitivity: what the toleranced mode is held to ----------------------------------------------------------
DRAWS = 4                    # independent perturbations per case
PERTURBATION = 2.0 ** -16    # relative, per texel, channel and frame: the size class of one rounding of a 1e-5-accurate weight
S_FLOOR = 2.0 ** -20         # a sensitivity below this is taken as this (an output that no colour input reaches, e-sky-all-out3)
BUDGET = 4.0                 # fast mode: Q <= BUDGET * max(S, S_FLOOR); reasons in DESIGN.md, "Reconstruction chain"
ILL_CONDITIONED = 3e-2       # a frame whose own Smax exceeds this: its maximum means nothing, only Q50 and Q99 are judged
SMALL_IMAGE = 256            # fewer pixels: the quantiles of a handful of channels are noise, only Qmax over the sequence is judged


def rel_err(a, b):
    """e(a, b) = |a - b| / (|b| + 1e-3) per colour channel: the measure of the header's stated tolerance."""
    a, b = np.asarray(a, np.float64)[..., :3], np.asarray(b, np.float64)[..., :3]
    return np.abs(a - b) / (np.abs(b) + 1e-3)


def quantiles(e):
    """(median, 99th percentile, maximum) of an array of errors; zeros for an empty one."""
    e = np.asarray(e).ravel()
    return (float(np.median(e)), float(np.percentile(e, 99)), float(e.max())) if e.size else (0.0, 0.0, 0.0)


def perturbed_frames(name, draw):
    """The case's frames with the .rgb of indirect, direct and albedo multiplied by float32(1 + u), u uniform in [-2^-16, 2^-16],
    independently per texel, channel and frame.  normal_depth and the cameras are untouched, so every decision of the chain that
    does not read a colour is the unperturbed run's."""
    rng = np.random.default_rng([sorted(CASES).index(name), draw])
    out = []
    for fc, cam, prev, planes in CASES[name]().frames:
        p = {k: v.copy() for k, v in planes.items()}
        for k in ("indirect", "direct", "albedo"):
            u = rng.uniform(-PERTURBATION, PERTURBATION, p[k][..., :3].shape)
            p[k][..., :3] *= (1.0 + u).astype(np.float32)
        out.append((fc, cam, prev, p))
    return out


@functools.lru_cache(maxsize=None)
def sensitivity(name):
    """-> float64 array (frames, 3): per frame S50, S99, Smax = the median, 99th percentile and maximum of
    e(oracle on perturbed colours, oracle_outputs), each the largest over the DRAWS draws."""
    c = CASES[name]()
    exact = oracle_outputs(name)
    s = np.zeros((len(exact), 3))
    for draw in range(DRAWS):
        got = run_oracle(c.w, c.h, c.settings, perturbed_frames(name, draw))
        s = np.maximum(s, [quantiles(rel_err(g, b)) for g, b in zip(got, exact)])
    s.setflags(write=False)
    return s
