"""Scenes and float64 references for the radiometry tests of the EXT shading model (tests/test_ext_radiometry.py on the CPU,
tests/test_ext_radiometry_gpu.py): what DESIGN.md "EXT shading model" states, integrated independently of both implementations.

  * `albedo(mu, material)`: E(mu) = integral over the upper hemisphere of (kd/pi + ks D G / (4 (n.wo)(n.wi))) (n.wi), the
    textbook form of DESIGN.md's formula (NOT the cancelled form ext_bsdf evaluates), by Gauss-Legendre quadrature over the half
    vector; `spec_albedo_direct` is the same integral over (theta, phi) of wi, the cross-check of the change of variables.
  * `far_furnace(material)`: a small plate with the material under test at the centre of a large emissive box.  Every direction
    above the plate sees radiance 1 from at least 9.8 away, so at depth 0 direct = E(mu) and at depth 1 indirect = 0.5 E(mu) on a
    plate pixel.
  * `lamp_scene(size)`: a coloured Lambert floor under two lamps of different emission, area, tilt and tessellation, the lamps in
    meshes that are not neighbours; `floor_direct` integrates the rectangles (not the tessellation) in float64.
  * `hard_table_scene(length)`: light tables of a given length whose areas span six orders of magnitude, with runs of zero-area
    entries: the binary search of the HIP side against the oracle's linear scan.

The estimator's error falls with the number of PIXELS averaged, not with frames (same section: one scalar per 16 frames
is added to all four channels of a blue-noise texel), so every statistic here is a mean over many pixels."""
import functools

import numpy as np

import pair_cull_support as S

F64 = np.float64

# The relative bounds of both test files (how they were chosen: tests/test_ext_radiometry.py, DESIGN.md "EXT shading model")
B_FURNACE = 0.03     # plate-wide means and the means over the two halves of the plate, direct and indirect
B_LAMP_TOTAL = 0.02  # floor-wide sum of direct
B_LAMP_BAND = 0.03   # its sums over the four distance bands


# ------------------------------------------------------------------------------------------------
# materials: rows of CapMaterial (kd, roughness, ks, -, ke, -)
# ------------------------------------------------------------------------------------------------
def material(kd=0.0, roughness=1.0, ks=0.0, ke=0.0):
    row = np.zeros(12, np.float32)
    row[0:3], row[3], row[4:7], row[8:11] = kd, roughness, ks, ke
    return row


def alpha_of(roughness):
    """alpha = max(roughness^2, 1e-3)"""
    return max(float(np.float32(roughness)) ** 2, 1e-3)


FURNACE_WALL = material(kd=0.5, ke=1.0)
FURNACE_MATERIALS = {
    "lambert": material(kd=0.5),
    "ggx r1": material(roughness=1.0, ks=1.0),
    "ggx r0.45": material(roughness=0.45, ks=1.0),
    "ggx r0.3": material(roughness=0.3, ks=1.0),
    "mix r0.6": material(kd=0.3, roughness=0.6, ks=0.6),
    "ggx r2": material(roughness=2.0, ks=1.0),
    "coloured ks r0.45": material(kd=0.3, roughness=0.45, ks=(0.9, 0.5, 0.2)),
}
EXTREME_MATERIALS = {
    "ggx r0": material(roughness=0.0, ks=1.0),
    "ggx r0.05": material(roughness=0.05, ks=1.0),
    "ggx r-0.7": material(roughness=-0.7, ks=1.0),
    "ggx r0.7": material(roughness=0.7, ks=1.0),
    "black": material(),
}


# ------------------------------------------------------------------------------------------------
# E(mu): float64 quadrature of the stated BSDF
# ------------------------------------------------------------------------------------------------
def _smith_g1(c, a2):
    return 2.0 * c / (c + np.sqrt(a2 + (1.0 - a2) * c * c))


def _ggx_d(ch, a2):
    return a2 / (np.pi * (ch * ch * (a2 - 1.0) + 1.0) ** 2)


@functools.lru_cache(None)
def _gauss(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w  # nodes and weights on [0, 1]


def spec_albedo_direct(mu, alpha, n=1500):
    """integral of D G / (4 (n.wo)(n.wi)) (n.wi) over the directions wi of the upper hemisphere, Gauss-Legendre in theta and phi
    (phi over half the circle: the integrand is even in it).  Resolves the lobe down to alpha = 0.09 (roughness 0.3) at n = 1500."""
    a2 = alpha * alpha
    x, w = _gauss(n)
    th, wth = x * (np.pi / 2), w * (np.pi / 2)
    ph, wph = x * np.pi, w * np.pi
    st, ct = np.sin(th)[:, None], np.cos(th)[:, None]
    so = np.sqrt(1.0 - mu * mu)
    hx, hy, hz = so + st * np.cos(ph)[None], st * np.sin(ph)[None], mu + ct
    ch = hz / np.sqrt(hx * hx + hy * hy + hz * hz)
    f = _ggx_d(ch, a2) * _smith_g1(mu, a2) * _smith_g1(ct, a2) / (4.0 * mu * ct)
    return 2.0 * float(wth @ (f * ct * st) @ wph)


def spec_albedo(mu, alpha, n=384):
    """The same integral over the half vector: wi = 2 (wo.h) h - wo, d wi = 4 (wo.h) dh, and the polar angle of h through
    r = integral of D (n.h) (cos^2 = (1 - r) / (1 + (alpha^2 - 1) r)), which flattens the lobe for every alpha; r = 1 - s^2 takes the
    1 / (n.h) of the horizon out.  Left: G (wo.h) / ((n.wo)(n.h)) where wo.h > 0 and n.wi > 0, over s in [0, 1] and phi."""
    a2 = alpha * alpha
    x, w = _gauss(n)
    s, ws = x[:, None], (w * 2.0 * x)[:, None]      # dr = 2 s ds
    ph, wph = x[None] * np.pi, w[None]              # d phi / (2 pi), both halves of the circle
    r = 1.0 - s * s
    c2 = (1.0 - r) / (1.0 + (a2 - 1.0) * r)
    ch, sh = np.sqrt(c2), np.sqrt(np.maximum(0.0, 1.0 - c2))
    so = np.sqrt(1.0 - mu * mu)
    woh = so * sh * np.cos(ph) + mu * ch
    ci = 2.0 * woh * ch - mu
    ok = (woh > 0.0) & (ci > 0.0)
    with np.errstate(all="ignore"):
        g = _smith_g1(mu, a2) * _smith_g1(np.where(ok, ci, 1.0), a2) * woh / (mu * ch)
    return float((ws * np.where(ok, g, 0.0) * wph).sum())


MU_LO, MU_HI, MU_NODES = 0.12, 0.75, 20


@functools.lru_cache(None)
def spec_table(alpha, n=384):
    """Chebyshev interpolant of spec_albedo(mu, alpha) over [MU_LO, MU_HI] (the plate's n.wo lie in 0.2 .. 0.6)"""
    k = np.arange(MU_NODES)
    t = np.cos(np.pi * (2 * k + 1) / (2 * MU_NODES))
    mu = 0.5 * (MU_LO + MU_HI) + 0.5 * (MU_HI - MU_LO) * t
    return np.polynomial.chebyshev.chebfit(t, [spec_albedo(m, alpha, n) for m in mu], MU_NODES - 1)


def spec_albedo_table(mu, alpha):
    mu = np.asarray(mu, F64)
    assert mu.size == 0 or (mu.min() >= MU_LO and mu.max() <= MU_HI)
    return np.polynomial.chebyshev.chebval((2.0 * mu - (MU_LO + MU_HI)) / (MU_HI - MU_LO), spec_table(alpha))


def albedo(mu, mat):
    """E(mu) per colour channel, [..., 3], for a material row: kd + ks * spec_albedo (the Lambert term integrates to kd exactly)"""
    mat = np.asarray(mat, F64)
    spec = spec_albedo_table(mu, alpha_of(mat[3])) if mat[4:7].any() else np.zeros(np.shape(mu))
    return mat[0:3] + mat[4:7] * np.asarray(spec)[..., None]


# ------------------------------------------------------------------------------------------------
# scenes from arrays (pair_cull_support's faces; any number of triangles)
# ------------------------------------------------------------------------------------------------
def assemble(groups):
    """groups: [(material row, [faces])] -> ((positions, normals, texcoords, indices, meshes), materials); one mesh per group, in
    order, as pair_cull_support.assemble lays them out (which stops at 64 triangles)"""
    pos, nrm, uv, idx, meshes, mats = [], [], [], [], [], []
    for slot, (mat, faces) in enumerate(groups):
        v_first, i_first, local = len(pos), len(idx), 0
        for kind, corners, n in faces:
            pos += list(corners)
            nrm += [n] * len(corners)
            uv += [(0, 0), (1, 0), (1, 1), (0, 1)][:len(corners)]
            idx += [local + k for k in {"fan": (0, 1, 2, 0, 2, 3), "split": (0, 1, 2, 2, 3, 0), "tri": (0, 1, 2)}[kind]]
            local += len(corners)
        meshes.append([len(pos) - v_first, v_first, len(idx) - i_first, i_first, slot, 0xFFFFFFFF, 0, 0])
        mats.append(mat)
    return (np.float32(pos), np.float32(nrm), np.float32(uv), np.uint32(idx), np.uint32(meshes)), np.float32(mats)


class Scene:
    """arrays, materials, camera and what the builder knows: `emissive` / `total` triangle counts, the lamps' rectangles"""

    def __init__(self, name, arrays, mats, cam, **info):
        self.name, self.arrays, self.mats, self.cam, self.info = name, arrays, mats, cam, info
        emissive = S.emissive_triangles(arrays[4], mats)
        self.emissive, self.total = int(emissive.sum()), len(emissive)

    def oracle(self):
        from oracle import cap_oracle as O
        return O.Scene(*self.arrays, materials=self.mats)


def look_at(position, target, w, h, focal, sensor_x=0.036):
    """the reference's camera basis (input_system.cpp:134-141: right = -forward x (0, 1, 0), up = forward x right)"""
    f = F64(target) - F64(position)
    f /= np.linalg.norm(f)
    right = -np.cross(f, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    return S.Cam(position, f, right, np.cross(f, right), focal, sensor_x, w, h)


def primary_dirs(cam, frame):
    """[h, w, 3] float64 directions of a frame's camera rays: create_primary_ray's formula (pixel + the frame's Halton jitter through
    the sensor), checked against oracle.primary_ray on a diagonal of pixels"""
    from oracle import cap_oracle as O
    jx, jy = S.jitter(frame)
    ys, xs = np.mgrid[0:cam.h, 0:cam.w]
    cx = ((xs + jx) / cam.w - 0.5) * float(cam.sx)
    cy = ((ys + jy) / cam.h - 0.5) * float(cam.sy)
    d = cx[..., None] * F64(cam.right) + cy[..., None] * F64(cam.up) + float(cam.focal) * F64(cam.forward)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    for k in range(0, min(cam.w, cam.h), 7):
        _, ref = O.primary_ray(cam.oracle(), k, k, cam.w, cam.h, frame)
        assert np.abs(d[k, k] - ref).max() < 1e-6
    return d


def mesh_ids(gbuffer_geo):
    return np.ascontiguousarray(gbuffer_geo[..., 2], np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# the far furnace
# ------------------------------------------------------------------------------------------------
FURNACE_W, FURNACE_H, FURNACE_FRAMES = 256, 256, 64
PLATE_HALF, BOX_HALF = 0.2, 10.0
# A wall point sees the plate, which emits nothing, under at most area * cos / (pi d^2) <= 0.16 / (pi 9.8^2) = 5.3e-4 of its
# cosine-weighted hemisphere; a wall point at the same height as the plate (cos = 0) or straight above it (9.8 .. 10 away) less.
# The plate sees only walls.  Both terms are far inside every bound below.
FURNACE_PLATE_SHADOW = 4 * PLATE_HALF ** 2 / (np.pi * (BOX_HALF - PLATE_HALF) ** 2)


def plate_faces():
    """the plate as a fan of six triangles about an off-centre point; two of them are slivers (2 and 3 mm wide at the rim)"""
    c = F64((0.05, 0.0, -0.03))
    a = PLATE_HALF
    rim = [(-a, 0, -a), (a, 0, -a), (a, 0, a), (a - 0.002, 0, a), (-a, 0, a), (-a, 0, a - 0.003)]
    return [S.tri([c, F64(rim[(k + 1) % 6]), F64(rim[k])], (0, 1, 0)) for k in range(6)]


@functools.lru_cache(None)
def far_furnace(name, w=FURNACE_W, h=FURNACE_H):
    mat = {**FURNACE_MATERIALS, **EXTREME_MATERIALS}[name]
    arrays, mats = assemble([(mat, plate_faces()), (FURNACE_WALL, S.box((-BOX_HALF,) * 3, (BOX_HALF,) * 3))])
    cam = look_at((0.0, 0.15, 0.4), (0.0, 0.0, 0.0), w, h, focal=0.06)
    return Scene("far furnace, " + name, arrays, mats, cam, plate_mesh=0)


# ------------------------------------------------------------------------------------------------
# the lamp scene
# ------------------------------------------------------------------------------------------------
LAMP_W, LAMP_H, LAMP_FRAMES = 192, 144, 16
FLOOR = material(kd=(0.8, 0.6, 0.4))
PANEL = material(kd=0.5)
KE_A, KE_B = (4.0, 2.0, 1.0), (1.0, 3.0, 9.0)
# rectangles as (centre, half edge u, half edge v): lamp A 1.0 x 0.6, horizontal, 1 above the floor; lamp B 0.3 x 0.3, tilted by 60 degrees
LAMP_A = (F64((-0.3, 1.0, 0.0)), F64((0.5, 0.0, 0.0)), F64((0.0, 0.0, 0.3)))
_C60, _S60 = np.cos(np.pi / 3), np.sin(np.pi / 3)
LAMP_B = (F64((0.9, 0.6, 0.0)), 0.15 * F64((_C60, -_S60, 0.0)), F64((0.0, 0.0, 0.15)))
LAMP_SIZES = {"lds table": (12, 1), "global table": (18, 1), "tree": (25, 6)}  # strips along x, cells across z of lamp A


def rect_normal(rect):
    n = np.cross(rect[1], rect[2])
    return n / np.linalg.norm(n)


def strip_quads(rect, strips, cells, ratio=0.8):
    """the rectangle as `strips` strips along u whose widths fall geometrically by `ratio`, each cut into `cells` quads along v"""
    c, u, v = rect
    n = -rect_normal(rect) if rect_normal(rect)[1] > 0 else rect_normal(rect)
    widths = ratio ** np.arange(strips)
    edges = np.concatenate([[0.0], np.cumsum(widths) / widths.sum()]) * 2.0 - 1.0
    out = []
    for k in range(strips):
        for j in range(cells):
            s0, s1, t0, t1 = edges[k], edges[k + 1], 2.0 * j / cells - 1.0, 2.0 * (j + 1) / cells - 1.0
            out.append(S.fan([c + s0 * u + t0 * v, c + s1 * u + t0 * v, c + s1 * u + t1 * v, c + s0 * u + t1 * v], n))
    return out


def zero_area(p, q, n):
    """a triangle with two equal vertices: area exactly 0 in any precision"""
    return S.tri([F64(p), F64(q), F64(q)], n)


@functools.lru_cache(None)
def lamp_scene(size, ke_a=KE_A, ke_b=KE_B, w=LAMP_W, h=LAMP_H):
    """mesh 0 floor, 1 lamp A (strips, a zero-area triangle in the middle and one as the last), 2 a panel that emits nothing (above
    both lamps: it shadows no floor point), 3 lamp B: the emissive triangle ids are not contiguous"""
    strips, cells = LAMP_SIZES[size]
    quads = strip_quads(LAMP_A, strips, cells)
    c, u, v = LAMP_A
    half = len(quads) // 2
    lamp_a = quads[:half] + [zero_area(c, c + 0.1 * u, (0, -1, 0))] + quads[half:] + [zero_area(c - u - v, c + u + v, (0, -1, 0))]
    nb = rect_normal(LAMP_B)
    nb = -nb if nb[1] > 0 else nb
    groups = [(FLOOR, [S.rect((0.2, 0.0, 0.0), (4.0, 0, 0), (0, 0, 4.0), (0, 1, 0))]),
              (material(kd=0.5, ke=ke_a), lamp_a),
              (PANEL, [S.rect((0.0, 2.5, 0.0), (0.8, 0, 0), (0, 0, 0.8), (0, -1, 0))]),
              (material(kd=0.5, ke=ke_b), [S.rect(LAMP_B[0], LAMP_B[1], LAMP_B[2], nb)])]
    arrays, mats = assemble(groups)
    cam = look_at((0.1, 1.7, 2.4), (0.1, 0.0, -0.1), w, h, focal=0.042)
    name = "lamp scene, %s" % size + ("" if (ke_a, ke_b) == (KE_A, KE_B) else ", ke %s %s" % (ke_a, ke_b))
    sc = Scene(name, arrays, mats, cam, floor_mesh=0, lamps=((LAMP_A, ke_a), (LAMP_B, ke_b)))
    assert sc.emissive == 2 * strips * cells + 4 and sc.total == sc.emissive + 4
    return sc


def floor_points(cam, frame):
    """[h, w, 3] float64: where a frame's camera rays meet the plane y = 0"""
    d = primary_dirs(cam, frame)
    o = F64(cam.position)
    t = -o[1] / d[..., 1]
    return o + t[..., None] * d


def rect_irradiance(points, rect, n=12):
    """integral over the rectangle of cos_s |cos_l| / d^2 dA for receivers `points` [N, 3] with normal +y: Gauss-Legendre n x n over
    the rectangle itself (emission is two-sided: |cos_l|).  A receiver is on one side of the lamp's plane for the whole lamp, so the
    integrand is smooth; the nearest lamp point is 0.4 from the floor."""
    c, u, v = rect
    nl = rect_normal(rect)
    x, w = _gauss(n)
    s, t = np.meshgrid(2.0 * x - 1.0, 2.0 * x - 1.0, indexing="ij")
    q = c + s.reshape(-1, 1) * u + t.reshape(-1, 1) * v
    wq = (np.outer(w, w) * 4.0 * np.linalg.norm(np.cross(u, v))).ravel()
    out = np.zeros(len(points))
    for a in range(0, len(points), 4096):
        L = q[None] - points[a:a + 4096, None]
        d2 = (L * L).sum(-1)
        out[a:a + 4096] = ((np.maximum(L[..., 1], 0.0) * np.abs(L @ nl) / (d2 * d2)) @ wq)
    return out


def floor_direct(points, lamps, kd, n=12):
    """expected `direct` at floor points [N, 3]: kd / pi * sum over the lamps of ke * rect_irradiance, [N, 3]"""
    out = np.zeros((len(points), 3))
    for rect, ke in lamps:
        out += rect_irradiance(points, rect, n)[:, None] * F64(ke)
    return out * F64(kd) / np.pi


def segments_cross(points, targets, rect):
    """number of segments point -> target that cross the rectangle (float64; every point against every target)"""
    c, u, v = rect
    nl = rect_normal(rect)
    seg = targets[None] - points[:, None]
    den = seg @ nl
    with np.errstate(all="ignore"):
        t = ((c - points) @ nl)[:, None] / den
        x = points[:, None] + t[..., None] * seg - c
        inside = (np.abs(x @ u) <= (u @ u) * (1 + 1e-9)) & (np.abs(x @ v) <= (v @ v) * (1 + 1e-9))
    return int(((den != 0) & (t > 0) & (t < 1) & inside).sum())


def rect_samples(rect, n=5):
    c, u, v = rect
    g = np.linspace(-1.0, 1.0, n)
    return np.array([c + a * u + b * v for a in g for b in g])


def assert_lamps_do_not_shadow(points):
    """no segment from a floor point in view to one lamp crosses the other lamp (or the panel): the direct term is unoccluded"""
    panel = (F64((0.0, 2.5, 0.0)), F64((0.8, 0, 0)), F64((0, 0, 0.8)))
    for lamp, others in ((LAMP_A, (LAMP_B, panel)), (LAMP_B, (LAMP_A, panel))):
        for other in others:
            assert segments_cross(points, rect_samples(lamp), other) == 0


# ------------------------------------------------------------------------------------------------
# hard light tables
# ------------------------------------------------------------------------------------------------
HARD_LENGTHS = (1, 2, 31, 32, 33, 64)


@functools.lru_cache(None)
def hard_table_scene(length, w=64, h=48):
    """Floor and one lamp mesh of `length` emissive triangles over lamp A's rectangle: right triangles in a row whose bases fall
    geometrically from 1 to 1e-6 (areas over six orders of magnitude), and zero-area
    triangles first, in a run of three after the tenth, and as the last two (equal prefix sums; the last entry is what a target at
    the total area falls back to).  Length 2: one triangle and a zero-area one; length 1: one triangle."""
    zeros = {1: (), 2: (1,)}.get(length, (0, 10, 11, 12, length - 2, length - 1))
    live = length - len(zeros)
    widths = 10.0 ** (-6.0 * np.arange(live) / max(1, live - 1))
    c, u, v = LAMP_A
    x = np.concatenate([[0.0], np.cumsum(widths) / widths.sum()]) * 2.0 - 1.0
    faces, k = [], 0
    for i in range(length):
        if i in zeros:
            faces.append(zero_area(c + x[k] * u, c + x[k] * u + v, (0, -1, 0)))
        else:
            faces.append(S.tri([c + x[k] * u - v, c + x[k + 1] * u - v, c + x[k] * u + v], (0, -1, 0)))
            k += 1
    arrays, mats = assemble([(FLOOR, [S.rect((0.2, 0.0, 0.0), (4.0, 0, 0), (0, 0, 4.0), (0, 1, 0))]), (material(kd=0.5, ke=KE_A), faces)])
    cam = look_at((0.1, 1.7, 2.4), (0.1, 0.0, -0.1), w, h, focal=0.042)
    sc = Scene("hard table, %d lights" % length, arrays, mats, cam, zeros=zeros)
    assert sc.emissive == length
    return sc


def light_table(scene):
    """(prefix sums, total) as both sides build them: fp32 areas |e1 x e2| / 2 in triangle order, fp32 running sum"""
    t = S.triangles(scene.arrays[0], scene.arrays[3], scene.arrays[4])[S.emissive_triangles(scene.arrays[4], scene.mats)]
    n = np.asarray(S.cross32(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])).reshape(-1, 3)
    area, cdf = np.float32(0), []
    for k in range(len(t)):
        area = np.float32(area + np.float32(0.5) * np.float32(np.sqrt(S.dot32(n[k], n[k]))))
        cdf.append(area)
    return np.float32(cdf), area


# ------------------------------------------------------------------------------------------------
# the oracle's frames, computed once per process and shared by the tests
# ------------------------------------------------------------------------------------------------
_MEANS, _FRAMES = {}, {}


def oracle_means(scene, bluenoise, frames, depth, threads=8):
    """mean over `frames` of the oracle's direct and indirect planes, the pixels whose camera ray meets mesh 0 in EVERY frame, the
    summed ray counters, how many camera rays met mesh 0 over all frames (`hits0`) and whether every plane of every frame was finite"""
    key = (scene.name, scene.cam.w, scene.cam.h, frames, depth)
    if key not in _MEANS:
        from oracle import cap_oracle as O
        sc, cam = scene.oracle(), scene.cam.oracle()
        direct = np.zeros((scene.cam.h, scene.cam.w, 3))
        indirect = np.zeros_like(direct)
        on0 = np.ones((scene.cam.h, scene.cam.w), bool)
        rays, finite, hits0 = np.zeros(3, np.int64), True, 0
        for f in range(frames):
            out = sc.render_frame(cam, bluenoise, scene.cam.w, scene.cam.h, f, depth, flags=O.FLAG_EXT_MATERIALS, threads=threads)
            direct += out["direct"][..., :3]
            indirect += out["indirect"][..., :3]
            on0 &= mesh_ids(out["gbuffer_geo"]) == 0
            hits0 += int((mesh_ids(out["gbuffer_geo"]) == 0).sum())
            rays += out["rays"]
            finite = finite and all(np.isfinite(out[k]).all() for k in ("direct", "indirect", "combined", "normal_depth", "albedo"))
        _MEANS[key] = dict(direct=direct / frames, indirect=indirect / frames, on0=on0, rays=tuple(int(r) for r in rays), finite=finite,
                           hits0=hits0)
    return _MEANS[key]


def oracle_frame(scene, bluenoise, frame, depth, threads=8):
    key = (scene.name, scene.cam.w, scene.cam.h, frame, depth)
    if key not in _FRAMES:
        from oracle import cap_oracle as O
        _FRAMES[key] = scene.oracle().render_frame(scene.cam.oracle(), bluenoise, scene.cam.w, scene.cam.h, frame, depth,
                                                   flags=O.FLAG_EXT_MATERIALS, threads=threads)
    return _FRAMES[key]


@functools.lru_cache(None)
def plate_mu(name, frames=FURNACE_FRAMES, w=FURNACE_W, h=FURNACE_H):
    """[frames, h, w] n.wo of the camera rays on the plate's plane (n = +y)"""
    cam = far_furnace(name, w, h).cam
    return np.stack([-primary_dirs(cam, f)[..., 1] for f in range(frames)])


def furnace_expected(name, frames=FURNACE_FRAMES, w=FURNACE_W, h=FURNACE_H):
    """[h, w, 3]: E(mu) of the material, averaged over the frames' jittered rays (valid on plate pixels)"""
    mu = np.clip(plate_mu("lambert", frames, w, h), MU_LO, MU_HI)  # the camera is the same for every material; off-plate pixels are not used
    return albedo(mu, far_furnace(name, w, h).mats[0]).mean(0)


@functools.lru_cache(None)
def lamp_irradiance(frames=LAMP_FRAMES, w=LAMP_W, h=LAMP_H, n=8):
    """[2, h, w]: rect_irradiance of lamp A and of lamp B at the floor point under each pixel, averaged over the frames' jittered rays
    (the three sizes and every ke share the rectangles and the camera), and [h, w] the floor distance of the pixel's point (frame 0)
    from the point under lamp A's centre"""
    cam = lamp_scene("lds table", KE_A, KE_B, w, h).cam
    out = np.zeros((2, h, w))
    for f in range(frames):
        p = floor_points(cam, f).reshape(-1, 3)
        for k, rect in enumerate((LAMP_A, LAMP_B)):
            out[k] += rect_irradiance(p, rect, n).reshape(h, w)
    p0 = floor_points(cam, 0)
    return out / frames, np.hypot(p0[..., 0] - LAMP_A[0][0], p0[..., 2] - LAMP_A[0][2])


def lamp_expected(ke_a=KE_A, ke_b=KE_B, frames=LAMP_FRAMES, w=LAMP_W, h=LAMP_H):
    """[h, w, 3] expected `direct` of the floor under each pixel, kd / pi * (ke_A I_A + ke_B I_B), and the distance of lamp_irradiance"""
    irr, dist = lamp_irradiance(frames, w, h)
    return (irr[0][..., None] * F64(ke_a) + irr[1][..., None] * F64(ke_b)) * F64(FLOOR[0:3]) / np.pi, dist


# ------------------------------------------------------------------------------------------------
# the statistics the tests bound: relative deviations of pixel means from the float64 values
# ------------------------------------------------------------------------------------------------
def furnace_deviations(direct, indirect, on_plate, name, frames=FURNACE_FRAMES):
    """direct, indirect: [h, w, 3] means over the frames; on_plate: the plate's pixels.  Returns per channel the relative deviation
    of the plate-wide mean of direct from E and of indirect from 0.5 E, and the same over the halves of the plate below and above
    the median n.wo (`direct_lo`, `direct_hi`, `indirect_lo`, `indirect_hi`)."""
    h, w = on_plate.shape
    e = furnace_expected(name, frames, w, h)
    mu = plate_mu("lambert", frames, w, h).mean(0)
    lo = on_plate & (mu < np.median(mu[on_plate]))
    out = {}
    for tag, sel in (("", on_plate), ("_lo", lo), ("_hi", on_plate & ~lo)):
        out["direct" + tag] = direct[sel].mean(0) / e[sel].mean(0) - 1.0
        out["indirect" + tag] = indirect[sel].mean(0) / (0.5 * e[sel].mean(0)) - 1.0
    return out


def lamp_deviations(direct, on_floor, ke_a=KE_A, ke_b=KE_B, frames=LAMP_FRAMES):
    """direct: [h, w, 3] mean over the frames; on_floor: the floor's pixels.  Returns per channel the relative deviation of the
    floor-wide sum from the integral (`total`) and of the sums over the four quartile bands of floor distance from the point under
    lamp A's centre (`bands`, [4, 3])."""
    h, w = on_floor.shape
    e, dist = lamp_expected(ke_a, ke_b, frames, w, h)
    band = np.digitize(dist, np.quantile(dist[on_floor], [0.25, 0.5, 0.75]))
    return dict(total=direct[on_floor].sum(0) / e[on_floor].sum(0) - 1.0,
                bands=np.stack([direct[on_floor & (band == b)].sum(0) / e[on_floor & (band == b)].sum(0) - 1.0 for b in range(4)]))
