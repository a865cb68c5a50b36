"""Models and scenes for the tests of the small-scene pair culls (tests/test_pair_culls.py on the CPU, tests/test_pair_culls_gpu.py).

The fused kernels of scenes of at most 64 triangles skip work on three decisions, each claimed to change no result bit:
  * the next-event pair cull of the EXT model (ctx_scene.hip update_nee_pairs): `nee_rule` restates its rule;
  * the camera pair cull of bounce 0 (small_scene.hip stage_camera_pairs / pair_mask, host gate in ctx_render.hip cull_camera_pairs): `camera_bounds` restates
    the bounds and the gate, `camera_truth` says which of the model's culls are wrong;
  * the occluder-first probes of the reference model: `probe_scores` restates the order they probe in.
Everything is numpy: fp32 where the code under test works in fp32 (fused multiply-adds where it writes fmaf), float64 where it works in
double and for the truth.  The builders make the scenes of both test files; every scene has at most 64 triangles."""
import functools

import numpy as np

TILE = 8
PAD = 2.0                    # pixels lds_bounds adds on every side
Z_MIN = np.float32(1e-4)     # a vertex at or behind this depth makes a pair cover the screen
F32 = np.float32

WALL = (0.7, 0.6, 0.5, 0.4, 0.04, 0.04, 0.04, 0.0, 0.0, 0.0, 0.0, 0.0)   # kd, roughness, ks, -, ke, - (test_two_phase_ext)
LAMP = (0.5, 0.5, 0.5, 1.0, 0.0, 0.0, 0.0, 0.0, 12.0, 11.0, 8.0, 0.0)


# ------------------------------------------------------------------------------------------------
# scenes: groups of faces -> one mesh per group (own vertex range, local indices), one material row per mesh
# ------------------------------------------------------------------------------------------------
def fan(corners, normal):
    """a quad triangulated as the fan (a, b, c), (a, c, d): folds into one fan pair"""
    return ("fan", [np.float64(c) for c in corners], np.float64(normal))


def split(corners, normal):
    """a quad triangulated as (a, b, c), (c, d, a): two loose triangles (different v0)"""
    return ("split", [np.float64(c) for c in corners], np.float64(normal))


def tri(corners, normal):
    return ("tri", [np.float64(c) for c in corners], np.float64(normal))


def rect(centre, u, v, normal, kind=fan):
    """the quad centre -+ u -+ v"""
    c, u, v = np.float64(centre), np.float64(u), np.float64(v)
    return kind([c - u - v, c + u - v, c + u + v, c - u + v], normal)


def grid(centre, u, v, nu, nv, normal, kind=fan):
    """the same rectangle as nu x nv quads"""
    c, u, v = np.float64(centre), np.float64(u), np.float64(v)
    out = []
    for j in range(nv):
        for i in range(nu):
            cc = c + u * ((2 * i + 1) / nu - 1.0) + v * ((2 * j + 1) / nv - 1.0)
            out.append(rect(cc, u / nu, v / nv, normal, kind))
    return out


def box(lo, hi, kind=fan, skip=()):
    """the six walls of [lo, hi] with inward normals, by name: floor, ceiling, back (-z), front (+z), left (-x), right (+x)"""
    lo, hi = np.float64(lo), np.float64(hi)
    c, e = (lo + hi) / 2, (hi - lo) / 2
    X, Y, Z = np.diag(e)
    walls = {"floor": (c - Y, X, Z, (0, 1, 0)), "ceiling": (c + Y, X, -Z, (0, -1, 0)), "back": (c - Z, X, Y, (0, 0, 1)),
             "front": (c + Z, -X, Y, (0, 0, -1)), "left": (c - X, Z, Y, (1, 0, 0)), "right": (c + X, -Z, Y, (-1, 0, 0))}
    return [rect(*walls[k], kind=kind) for k in walls if k not in skip]


def assemble(groups):
    """groups: [(material row, [faces])].  Returns ((positions, normals, texcoords, indices, meshes), materials)."""
    pos, nrm, uv, idx, meshes, mats = [], [], [], [], [], []
    for slot, (mat, faces) in enumerate(groups):
        v_first, i_first, local = len(pos), len(idx), 0
        for kind, corners, n in faces:
            pos += corners
            nrm += [n] * len(corners)
            uv += [(0, 0), (1, 0), (1, 1), (0, 1)][:len(corners)]
            order = {"fan": (0, 1, 2, 0, 2, 3), "split": (0, 1, 2, 2, 3, 0), "tri": (0, 1, 2)}[kind]
            idx += [local + k for k in order]
            local += len(corners)
        meshes.append([len(pos) - v_first, v_first, len(idx) - i_first, i_first, slot, 0xFFFFFFFF, 0, 0])
        mats.append(mat)
    arrays = (np.float32(pos), np.float32(nrm), np.float32(uv), np.uint32(idx), np.uint32(meshes))
    assert len(idx) // 3 <= 64
    return arrays, np.float32(mats)


def with_positions(arrays, positions):
    return (np.ascontiguousarray(positions, np.float32),) + tuple(arrays[1:])


def triangles(positions, indices, meshes):
    """(n, 3, 3) fp32 vertices in global triangle order: mesh-table order, then primitive order (cap_scene_upload's ids)"""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    indices = np.asarray(indices, np.int64).ravel()
    out = []
    for nv, v_first, ni, i_first in np.asarray(meshes, np.int64).reshape(-1, 8)[:, :4]:
        out.append(pos[v_first + indices[i_first:i_first + ni]].reshape(-1, 3, 3))
    return np.concatenate(out) if out else np.zeros((0, 3, 3), np.float32)


def fma32(a, b, c):
    """fmaf for fp32 operands: the product is exact in float64"""
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def dot32(a, b):
    """cap_math.h dot3"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def cross32(a, b):
    """cap_math.h cross3"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.stack([fma32(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])), fma32(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     fma32(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], -1)


def fan_records(positions, indices, meshes):
    """The fan pairs and loose triangles of the small-scene path, as upload_fan_records folds them (comment there): triangles k and
    k + 1 become one pair iff they have the same v0 and e2(k) == e1(k + 1), bit for bit, over the records k_tri_setup writes
    (v0, e1 = v1 - v0, e2 = v2 - v0, n = e1 x e2 in fp32).  Returns (pairs, singles): a pair is a dict with its first triangle id `tri`,
    v0, the edges e1, e2, e3 and the normals nA, nB; a single is a triangle id."""
    t = triangles(positions, indices, meshes)
    v0, e1, e2 = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    n = cross32(e1, e2)
    pairs, singles, k = [], [], 0
    while k < len(t):
        if k + 1 < len(t) and v0[k].tobytes() == v0[k + 1].tobytes() and e2[k].tobytes() == e1[k + 1].tobytes():
            pairs.append(dict(tri=k, v0=v0[k], e1=e1[k], e2=e2[k], e3=e2[k + 1], nA=n[k], nB=n[k + 1]))
            k += 2
        else:
            singles.append(k)
            k += 1
    return pairs, singles


# ------------------------------------------------------------------------------------------------
# the next-event pair cull
# ------------------------------------------------------------------------------------------------
def emissive_triangles(meshes, materials):
    """per global triangle: is the material of its mesh -- row `index` of the mesh table, column 4 -- emissive (cap_materials_upload)"""
    m = np.asarray(meshes, np.int64).reshape(-1, 8)
    mats = np.asarray(materials, np.float32).reshape(-1, 12)
    return np.repeat((mats[m[:, 4], 8:11] > 0).any(1), m[:, 2] // 3)


def nee_rule(positions, indices, meshes, materials, first_rule=False):
    """The rule above update_nee_pairs, in double over the uploaded vertices.  A pair is culled iff for both of its triangles, with
    plane (v0, n): (i) every scene vertex lies on one closed side of the plane, at most 2.5e-7 * Dv beyond it (Dv = the largest
    distance from v0 to a scene vertex), and (ii) every vertex of every light triangle (a triangle of a mesh whose ke is positive) is at
    least delta = 1e-2 * D * Dv on that side (D = the diagonal of the scene's box).  first_rule: the tolerance of (i) as the rule was
    first written, 1e-6 * D, which does not compose with (ii) (see nee_truth).  Returns a list with one dict per fan pair -- `culled`,
    `reason` it is kept (None, "no lights", "zero normal", "not hull", "light close"), `delta` and `dv` of the triangle that decided -- and
    (tested, pairs) as CAP_DEBUG_NEE_PAIRS packs them."""
    pairs, _ = fan_records(positions, indices, meshes)
    P = np.float64(np.ascontiguousarray(positions, np.float32).reshape(-1, 3))
    mats = np.asarray(materials, np.float32).reshape(-1, 12)
    t = triangles(positions, indices, meshes)
    emissive = emissive_triangles(meshes, mats)
    lights = np.float64(t[emissive].reshape(-1, 3))
    D = float(np.linalg.norm(P.max(0) - P.min(0))) if len(P) else 0.0
    out = []
    for p in pairs:
        res = dict(tri=p["tri"], culled=False, reason=None, delta=None, dv=None)
        out.append(res)
        if not len(lights) or not D > 0.0:
            res["reason"] = "no lights"
            continue
        v0 = np.float64(p["v0"])
        for n in (p["nA"], p["nB"]):
            n = np.float64(n)
            nl = float(np.sqrt((n * n).sum()))
            if not nl > 0.0:
                res["reason"] = "zero normal"
                break
            e = P - v0
            sd = (e @ n) / nl
            smin, smax = min(0.0, sd.min()), max(0.0, sd.max())
            dv = float(np.sqrt((e * e).sum(1)).max())
            res["delta"], res["dv"] = 1e-2 * D * dv, dv
            tol = 1e-6 * D if first_rule else 2.5e-7 * dv
            if smax <= tol:
                sign = -1.0
            elif smin >= -tol:
                sign = 1.0
            else:
                res["reason"] = "not hull"
                break
            if not (sign * (((lights - v0) @ n) / nl) >= res["delta"]).all():
                res["reason"] = "light close"
                break
        res["culled"] = res["reason"] is None
    kept = sum(1 for r in out if not r["culled"])
    return out, (kept, len(pairs))


def nee_counts(arrays, mats, first_rule=False):
    return nee_rule(arrays[0], arrays[3], arrays[4], mats, first_rule)[1]


def nee_truth(arrays, mats, first_rule=False, per_triangle=48, per_light=12, seed=3):
    """Next-event segments that a culled pair occludes, in float64: from points p on every triangle of the scene (corners, centroid,
    random points) to points y on every light triangle, a culled triangle reports an occlusion iff the segment crosses it at
    tmin = 1e-4 < t < 0.999 |y - p| (the intersection contract's interval).  Returns [(pair, p, y, t)]; empty for an exact cull.  With
    first_rule a point 1e-6 D outside a culled plane -- a decal on a hull wall -- crosses it at t = 1e-6 D |y - p| / delta, up to
    2e-4: inside the interval."""
    rule, _ = nee_rule(arrays[0], arrays[3], arrays[4], mats, first_rule)
    t = np.float64(triangles(arrays[0], arrays[3], arrays[4]))
    emissive = emissive_triangles(arrays[4], mats)
    rs = np.random.RandomState(seed)

    def points(tris, n):
        b = rs.dirichlet((1.0, 1.0, 1.0), (len(tris), n))
        b = np.concatenate([np.broadcast_to(np.eye(3), (len(tris), 3, 3)), np.full((len(tris), 1, 3), 1 / 3), b], 1)
        return np.einsum("tnk,tkx->tnx", b, tris).reshape(-1, 3)
    p, y = points(t, per_triangle), points(t[emissive], per_light)
    seg = y[None] - p[:, None]                       # [P, Y, 3]
    length = np.linalg.norm(seg, axis=-1)
    with np.errstate(all="ignore"):
        d = seg / length[..., None]
        out = []
        for k, r in enumerate(rule):
            if not r["culled"]:
                continue
            for tr in t[r["tri"]:r["tri"] + 2]:
                e1, e2 = tr[1] - tr[0], tr[2] - tr[0]
                pv = np.cross(d, e2)
                det = pv @ e1
                tv = (p - tr[0])[:, None]
                u = (tv * pv).sum(-1) / det
                qv = np.cross(tv, e1)
                v = (d * qv).sum(-1) / det
                tt = (qv @ e2) / det
                hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (tt > 1e-4) & (tt < 0.999 * length)
                for i, j in np.argwhere(hit)[:4]:
                    out.append((k, p[i], y[j], float(tt[i, j])))
    return out


# ------------------------------------------------------------------------------------------------
# cameras
# ------------------------------------------------------------------------------------------------
class Cam:
    """position, right, up, forward (fp32 rows), focal length and sensor size, as CapCameraData holds them"""

    def __init__(self, position, forward, right, up, focal, sensor_x, w, h):
        self.position, self.forward, self.right, self.up = (np.float32(a) for a in (position, forward, right, up))
        self.focal, self.sx = F32(focal), F32(sensor_x)
        self.sy = F32(sensor_x) * (F32(h) / F32(w))  # camera_system.cpp:10-17
        self.w, self.h = w, h

    def capi(self):
        from capsaicin_amd import capi
        cam = capi.CameraData()
        cam.position[:], cam.forward[:], cam.right[:], cam.up[:] = self.position, self.forward, self.right, self.up
        cam.focal_length, cam.sensor_size[0], cam.sensor_size[1] = self.focal, self.sx, self.sy
        return cam

    def oracle(self):
        from oracle import cap_oracle as O
        return O.make_camera(tuple(self.position), tuple(self.forward), tuple(self.right), tuple(self.up), self.sx, self.sy, self.focal)


def axis_camera(position, w, h, focal=0.03, sensor_x=0.036, right=(-1, 0, 0), up=(0, 1, 0), forward=(0, 0, -1)):
    return Cam(position, forward, right, up, focal, sensor_x, w, h)


def euler_camera(position, yaw, pitch, roll, w, h, focal=0.03, sensor_x=0.036):
    """an orthonormal basis from three angles, made in float64 and rounded to fp32 once; yaw 0 looks along -z like axis_camera"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.float64([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.float64([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.float64([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    M = Ry @ Rx @ Rz
    return Cam(position, M @ (0, 0, -1), M @ (-1, 0, 0), M @ (0, 1, 0), focal, sensor_x, w, h)


def camera_gate(cam):
    """cap_render's gate (ctx_render.hip cull_camera_pairs): the cull is on iff skew = max |Gram - I| of (right, up, forward) is below 1e-4 and the worst-case shift of a
    projected point on the sensor, skew * extent * (f / s + 1 + s' / (2 s) + (sx + sy) / (4 f)), is at most PAD / 8 in x and in y.
    Returns (gate, skew, shift_x, shift_y)."""
    def dotf(a, b):  # x[0] * y[0] + x[1] * y[1] + x[2] * y[2] in fp32, no contraction
        return F32(F32(a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])
    R, U, Fw = cam.right, cam.up, cam.forward
    skew = max(abs(dotf(R, U)), abs(dotf(R, Fw)), abs(dotf(U, Fw)), abs(dotf(R, R) - F32(1)), abs(dotf(U, U) - F32(1)), abs(dotf(Fw, Fw) - F32(1)))
    f, sx, sy = float(cam.focal), float(cam.sx), float(cam.sy)
    shift_x = float(skew) * cam.w * (f / sx + 1.0 + sy / (2.0 * sx) + (sx + sy) / (4.0 * f))
    shift_y = float(skew) * cam.h * (f / sy + 1.0 + sx / (2.0 * sy) + (sx + sy) / (4.0 * f))
    gate = bool(skew < F32(1e-4) and shift_x <= 0.125 * PAD and shift_y <= 0.125 * PAD)
    return (1 if gate else 0), float(skew), shift_x, shift_y


def pair_vertices(pair, position):
    """vertex - camera for the four vertices of a pair, with the kernel's fp32 steps (tvec = o - v0; -tvec, e - tvec)"""
    tvec = np.float32(position) - pair["v0"]
    return np.stack([-tvec, pair["e1"] - tvec, pair["e2"] - tvec, pair["e3"] - tvec])


def camera_bounds(arrays, cam, gate=None):
    """The screen bounds of every fan pair as k_trace_shade stages them in lds_bounds: each vertex projected with the TRANSPOSE of
    (right, up, forward) -- z = d.forward, pixel = ((f * d.right / z) / sensor + 0.5) * extent -- min / max over the four vertices,
    grown by PAD; (-3e38, -3e38, 3e38, 3e38) when the gate is 0, a vertex is not in front of z = 1e-4 (fp32 compare) or a bound is NaN.
    The depth is computed as the kernel does, in fp32; the rest in float64.  Returns (bounds [pairs, 4], gate, unpadded [pairs, 4])."""
    if gate is None:
        gate = camera_gate(cam)[0]
    pairs, _ = fan_records(arrays[0], arrays[3], arrays[4])
    R, U = np.float64(cam.right), np.float64(cam.up)
    f, sx, sy = float(cam.focal), float(cam.sx), float(cam.sy)
    bounds, raw = np.zeros((len(pairs), 4)), np.zeros((len(pairs), 4))
    for k, p in enumerate(pairs):
        d = pair_vertices(p, cam.position)
        z32 = dot32(d, cam.forward)
        behind = bool((~(z32 > Z_MIN)).any())
        with np.errstate(all="ignore"):
            z = np.float64(z32)
            px = ((f * (np.float64(d) @ R) / z) / sx + 0.5) * cam.w
            py = ((f * (np.float64(d) @ U) / z) / sy + 0.5) * cam.h
        raw[k] = (px.min(), py.min(), px.max(), py.max())
        usable = gate and not behind and not np.isnan(raw[k]).any()
        bounds[k] = raw[k] + (-PAD, -PAD, PAD, PAD) if usable else (-3.0e38, -3.0e38, 3.0e38, 3.0e38)
    return bounds, gate, raw


def tile_keeps(bounds, w, h):
    """[tiles_y, tiles_x, pairs]: the pairs a tile of camera rays tests (the `over` ballot of k_trace_shade)"""
    tx = np.arange((w + TILE - 1) // TILE)[None, :, None] * float(TILE)
    ty = np.arange((h + TILE - 1) // TILE)[:, None, None] * float(TILE)
    b = bounds[None, None]
    return (b[..., 0] < tx + TILE) & (b[..., 2] >= tx) & (b[..., 1] < ty + TILE) & (b[..., 3] >= ty)


def jitter(frame):
    """the sub-pixel sample position of a frame, from the oracle's frame constants"""
    from oracle import cap_oracle as O
    return tuple(float(x) for x in O.halton23(frame))


def camera_truth(arrays, cam, frames, gate=None):
    """Every (tile_y, tile_x, pair) the model culls although, in one of `frames`, a sample position of a pixel of that tile has a camera
    ray that meets the pair.  The truth projects with the general inverse of (right, up, forward) in float64: a ray through the sensor
    point c = (cx, cy, f) has direction B c, so a vertex d = B c' is seen at c' = B^-1 d; a sample meets a triangle iff it lies inside
    the triangle's projection (all vertices in front).  Empty for an exact cull."""
    bounds, gate, _ = camera_bounds(arrays, cam, gate)
    keeps = tile_keeps(bounds, cam.w, cam.h)
    pairs, _ = fan_records(arrays[0], arrays[3], arrays[4])
    Binv = np.linalg.inv(np.float64(np.stack([cam.right, cam.up, cam.forward], 1)))
    f, sx, sy = float(cam.focal), float(cam.sx), float(cam.sy)
    ys, xs = np.mgrid[0:cam.h, 0:cam.w]
    wrong = []
    for k, p in enumerate(pairs):
        if keeps[..., k].all():
            continue
        c = (Binv @ (np.float64(p["v0"]) + np.float64([np.zeros(3), p["e1"], p["e2"], p["e3"]]) - np.float64(cam.position)).T).T
        assert (c[:, 2] > 0).all()  # a culled pair is in front of the camera
        q = np.stack([(c[:, 0] * f / c[:, 2] / sx + 0.5) * cam.w, (c[:, 1] * f / c[:, 2] / sy + 0.5) * cam.h], 1)  # pixels
        hit = np.zeros((cam.h, cam.w), bool)
        for frame in frames:
            jx, jy = jitter(frame)
            s = np.stack([xs + jx, ys + jy], -1)
            for a, b, cc in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
                def edge(u, v):
                    return (v[0] - u[0]) * (s[..., 1] - u[1]) - (v[1] - u[1]) * (s[..., 0] - u[0])
                e0, e1, e2 = edge(a, b), edge(b, cc), edge(cc, a)
                hit |= ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        for ty in range(keeps.shape[0]):
            for tx in range(keeps.shape[1]):
                if not keeps[ty, tx, k] and hit[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].any():
                    wrong.append((ty, tx, k))
    return wrong


# ------------------------------------------------------------------------------------------------
# the probes' order
# ------------------------------------------------------------------------------------------------
def probe_scores(arrays, frame):
    """lds_pscore / lds_score: per fan pair the sum over its four vertices of vertex . light direction of the batch's first frame (fp32,
    the kernels' order of operations).  Returns (scores, order): order[0] is the pair probed first, ties go to the lower index."""
    from oracle import cap_oracle as O
    L = np.float32(O.directional_light(frame)[0])
    pairs, _ = fan_records(arrays[0], arrays[3], arrays[4])
    sc = []
    for p in pairs:
        s = dot32(p["v0"], L)
        for e in (p["e1"], p["e2"], p["e3"]):
            s = F32(s + dot32(p["v0"] + e, L))
        sc.append(s)
    sc = np.float32(sc)
    return sc, sorted(range(len(sc)), key=lambda k: (-sc[k], k))


# ------------------------------------------------------------------------------------------------
# the cases of both test files
# ------------------------------------------------------------------------------------------------
class Case:
    """one scene, one camera, the frames to render; `ext` says whether the scene has a light (EXT model possible); `expect` holds
    what the builder designed (checked on the CPU against the models, on the GPU against the debug keys)"""

    def __init__(self, name, arrays, mats, cam, frames=(0, 5), **expect):
        self.name, self.arrays, self.mats, self.cam, self.frames, self.expect = name, arrays, mats, cam, frames, expect


BOX_LO, BOX_HI = (-1.0, -1.0, -1.2), (1.0, 1.0, 1.2)
W, H = 72, 56


def lamp_quad(centre, half=0.3):
    return rect(centre, (half, 0, 0), (0, 0, half), (0, -1, 0))


def inner_quads():
    tilt = np.float64([0.3, 0.5, 0.8124])
    tilt /= np.linalg.norm(tilt)
    tu = np.cross(tilt, (0.0, 0.0, 1.0))
    tu /= np.linalg.norm(tu)
    tv = np.cross(tilt, tu)
    return [rect((0.1, -0.3, -0.2), 0.35 * tu, 0.35 * tv, tilt), rect((-0.55, -0.6, 0.3), (0.2, 0, 0), (0, 0.4, 0), (0, 0, 1))]


_CORNELL = {}


def cornell(scale):
    """N1: the Cornell box with its materials (tests/test_ext_gpu.py cornell_with_materials), every position and the camera's times
    `scale`: delta = 1e-2 D Dv goes with its square, the distances with the scale itself."""
    if "geo" not in _CORNELL:
        import os
        import shutil
        import tempfile
        from capsaicin_amd import capi
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if not os.path.exists(capi.LIB_PATH):
            capi.build_native()
        with tempfile.TemporaryDirectory() as tmp:
            txt = open(os.path.join(root, "assets", "cornell_box.obj")).read().replace("mtllib cornellbox.mtl", "mtllib cornell_box.mtl")
            open(os.path.join(tmp, "c.obj"), "w").write(txt)
            shutil.copy(os.path.join(root, "assets", "cornell_box.mtl"), os.path.join(tmp, "cornell_box.mtl"))
            geo = capi.Geometry(os.path.join(tmp, "c.obj"))
            _CORNELL["geo"] = ((geo.positions.copy(), geo.normals.copy(), geo.texcoords.copy(), geo.indices.copy(), geo.meshes.copy()),
                               geo.materials().copy(), capi.cornell_camera(W, H))
    arrays, mats, c = _CORNELL["geo"]
    arrays = with_positions(arrays, arrays[0] * F32(scale))
    cam = Cam(np.float32(c.position) * F32(scale), c.forward, c.right, c.up, c.focal_length, c.sensor_size[0], W, H)
    return Case("N1 cornell x%g" % scale, arrays, mats, cam, scale=scale)


def hanging(factor, name="N2"):
    """N2: a closed box, a lamp quad `factor` x delta of the ceiling pair below the ceiling"""
    def make(y):
        return assemble([(WALL, box(BOX_LO, BOX_HI)), (LAMP, [lamp_quad((0.0, y, 0.0))])])
    rule, _ = nee_rule(*[make(0.0)[0][k] for k in (0, 3, 4)], make(0.0)[1])
    delta = rule[1]["delta"]  # the ceiling is the second wall of box()
    arrays, mats = make(BOX_HI[1] - factor * delta)
    cam = euler_camera((0.1, -0.2, 1.0), 0.2, 0.35, 0.0, W, H)
    return Case("%s lamp %.4g delta below the ceiling" % (name, factor), arrays, mats, cam, ceiling_culled=factor > 1.0, delta=delta)


def decal(s=None, tol=None):
    """N3: a long room; its left wall (the plane x = 0) is two pairs, A (z 0..4) and B (z 4..8, v0 on the lamp's side, so that Dv is
    about half the room).  A decal outside the plane -- by s x 1e-6 D, the unit of the rule's first tolerance, or by tol x 2.5e-7 Dv(B),
    the unit of its tolerance now -- overlaps B from z = 7 and goes on to the front wall at z = 8.5, where it is the room's wall.  The
    lamp is 1.001 delta(B) inside the plane at the near end, so segments from the decal to the lamp are 1.5 Dv long and cross the plane
    up to 1.5e-4 s from where they start: those that start on the decal within that distance of B's edge cross B itself.  The camera
    looks at a millimetre of the wall around that edge.  B is culled while the decal is within the tolerance: tol < 1, s = 0."""
    def make(disp, lamp_x):
        walls = box((0, 0, 0), (1.5, 1.5, 8.5), skip=("left",))
        walls.append(fan([(0, 0, 0), (0, 0, 4), (0, 1.5, 4), (0, 1.5, 0)], (1, 0, 0)))           # A
        walls.append(fan([(0, 0, 4), (0, 0, 8), (0, 1.5, 8), (0, 1.5, 4)], (1, 0, 0)))           # B: pair 6
        walls.append(fan([(-disp, 0, 7.0), (-disp, 0, 8.5), (-disp, 1.5, 8.5), (-disp, 1.5, 7.0)], (1, 0, 0)))
        lamp = rect((lamp_x + 0.15, 1.2, 0.4), (0.15, 0, 0), (0, 0, 0.2), (0, -1, 0))
        return assemble([(WALL, walls), (LAMP, [lamp])])
    D = float(np.linalg.norm((1.5, 1.5, 8.5)))
    a, m = make(0.0, 0.5)
    flat = nee_rule(a[0], a[3], a[4], m)[0][6]
    disp = s * 1e-6 * D if tol is None else tol * 2.5e-7 * flat["dv"]
    a, m = make(disp, 0.5)
    delta = nee_rule(a[0], a[3], a[4], m)[0][6]["delta"]
    arrays, mats = make(disp, 1.001 * delta)
    cam = axis_camera((1.0, 0.75, 8.0002), W, H, focal=0.036 * 1044, forward=(-1, 0, 0), right=(0, 0, 1), up=(0, 1, 0))
    name = "N3 decal %.4g e-6 D outside" % s if tol is None else "N3 decal %.4g tolerances outside" % tol
    return Case(name, arrays, mats, cam, s=s, tol=tol, disp=disp, wall_pair=6, decal_tri=14,
                culled_first_rule=disp < 1e-6 * D, culled=(s == 0) if tol is None else tol < 1.0)


def corridor():
    """N4: the floor is three quads in a row (the middle one's Dv is about half the length), lamps at both ends"""
    hi = (0.6, 0.6, 3.0)
    walls = [rect((0.3, 0.0, 0.5 + k), (0.3, 0, 0), (0, 0, 0.5), (0, 1, 0)) for k in range(3)] + box((0, 0, 0), hi, skip=("floor",))
    lamps = [rect((0.3, 0.48, z), (0.1, 0, 0), (0, 0, 0.1), (0, -1, 0)) for z in (0.25, 2.75)]
    arrays, mats = assemble([(WALL, walls), (LAMP, lamps)])
    return Case("N4 corridor", arrays, mats, axis_camera((0.3, 0.3, 2.9), W, H, focal=0.02), floor_pairs=(0, 1, 2))


def kept_reasons():
    """N5: one pair per reason a pair stays in the list"""
    a, b, d = np.float64((-0.6, -0.2, -0.5)), np.float64((-0.2, -0.2, -0.5)), np.float64((-0.6, 0.3, -0.5))
    walls = box(BOX_LO, BOX_HI) + [fan([a, b, b, d], (0, 0, 1)), inner_quads()[0]]
    lamps = [lamp_quad((-0.3, BOX_HI[1], 0.0), 0.25), rect((0.95, 0.0, 0.3), (0, 0.2, 0), (0, 0, 0.2), (-1, 0, 0))]
    arrays, mats = assemble([(WALL, walls), (LAMP, lamps)])
    reasons = [None, "light close", None, None, None, "light close", "zero normal", "not hull", "light close", "not hull"]
    return Case("N5 kept reasons", arrays, mats, euler_camera((0.0, -0.1, 1.0), 0.25, 0.2, 0.0, W, H), reasons=reasons)


def room(extra=(), lamp=True, **kw):
    """the room of the camera cases: 6 walls, two quads inside, a lamp under the ceiling (9 pairs; + extra)"""
    groups = [(WALL, box(BOX_LO, BOX_HI, **kw) + inner_quads() + list(extra))]
    if lamp:
        groups.append((LAMP, [lamp_quad((0.3, 0.9, -0.2), 0.25)]))
    return assemble(groups)


def room_views():
    """C1: eight random orthonormal cameras (yaw, pitch, roll) inside the room, at 44 x 20 and 72 x 40 -- the first eight draws for
    which the model culls at least one (tile, pair) and keeps at least one at both sizes"""
    rs = np.random.RandomState(11)
    arrays, mats = room()
    out = []
    while len(out) < 16:
        pos = rs.uniform((-0.7, -0.5, -0.4), (0.7, 0.5, 0.9))
        yaw, pitch, roll = rs.uniform(-np.pi, np.pi), rs.uniform(-0.6, 0.6), rs.uniform(-0.5, 0.5)
        cams = [euler_camera(pos, yaw, pitch, roll, w, h) for w, h in ((44, 20), (72, 40))]
        keeps = [tile_keeps(camera_bounds(arrays, c)[0], c.w, c.h) for c in cams]
        if all(k.any() and not k.all() for k in keeps):
            out += [Case("C1 view %d at %dx%d" % (len(out) // 2, c.w, c.h), arrays, mats, c, gate=1) for c in cams]
    return out


def plane_cuts():
    """C2: the camera plane cuts through quads; a vertex one ulp to either side of the depth 1e-4; a camera 2e-4 in front of a wall"""
    out = []
    arrays, mats = room()
    out.append(Case("C2 side walls straddle the camera plane", arrays, mats, euler_camera((0.1, 0.05, 0.4), 0.5, 0.2, 0.1, W, H), gate=1))
    for name, z in (("below", np.nextafter(Z_MIN, F32(0))), ("above", np.nextafter(Z_MIN, F32(1)))):
        # camera at the origin looking along -z: the depth of v0 is exactly -v0.z
        near = fan([(2e-5, 1e-5, -float(z)), (0.3, 0.0, -0.5), (0.3, 0.3, -0.5), (0.0, 0.3, -0.5)], (0, 0, 1))
        a, m = room(extra=[near])
        out.append(Case("C2 vertex one ulp %s z = 1e-4" % name, a, m, axis_camera((0, 0, 0), W, H), gate=1, near_pair=8, near_behind=name == "below"))
    pos = (0.2, 0.1, BOX_LO[2] + 2e-4)
    out.append(Case("C2 facing a wall 2e-4 away", arrays, mats, axis_camera(pos, W, H), gate=1))
    out.append(Case("C2 oblique to a wall 2e-4 away", arrays, mats, euler_camera(pos, 1.0, 0.1, 0.0, W, H), gate=1))
    return out


def place_quad(cam, depth, x0, y0, x1, y1, normal=(0, 0, 1)):
    """a fan quad at `depth` along forward whose projection is the pixel rectangle (x0, y0) .. (x1, y1) for an orthonormal camera"""
    o, R, U, Fw = (np.float64(a) for a in (cam.position, cam.right, cam.up, cam.forward))
    def at(px, py):
        cx, cy = (px / cam.w - 0.5) * float(cam.sx), (py / cam.h - 0.5) * float(cam.sy)
        return o + (cx * R + cy * U + float(cam.focal) * Fw) * (depth / float(cam.focal))
    return fan([at(x0, y0), at(x1, y0), at(x1, y1), at(x0, y1)], normal)


def tile_edges():
    """C3: a quad whose edges lie -2.5, -1.5, -0.5 and +0.5 pixels beyond tile boundaries (outwards: the right edge at boundary + off,
    the left edge at boundary - off), inside the image and around the last, partial tile column and row of 44 x 20"""
    out = []
    w, h = 44, 20
    cam = axis_camera((0.0, 0.0, 1.0), w, h)
    for off in (-2.5, -1.5, -0.5, 0.5):
        for name, (bx0, by0, bx1, by1) in (("inner tiles", (16, 8, 32, 16)), ("last column and row", (8, 8, 40, 16))):
            target = (bx0 - off, by0 - off, bx1 + off, by1 + off)
            a, m = room(extra=[place_quad(cam, 1.5, *target)])
            out.append(Case("C3 edges %+.1f px, %s" % (off, name), a, m, cam, frames=(2, 7), gate=1, quad_pair=8, target=target))
    return out


def telephoto(eps_right, eps_up, name):
    """C4: forward (0, 0, -1); right = (-1, 0, 0) - eps_right forward, up = (0, 1, 0) - eps_up forward: every Gram term is below 1e-4, but
    with f / sensor_x = 700 at 72 x 16 the transposed projection is eps * 700 * 72 = 4.5 pixels off.  A quad at depth 10 whose true
    projection is x 23.1 .. 40.9, y 7.1 .. 8.9: in both directions a shift of 4.5 pixels pushes a bound, pad included, across a tile
    boundary (24, 40; 8) that the quad's samples reach."""
    w, h = 72, 16
    focal = 700 * 0.036
    true = axis_camera((0, 0, 0), w, h, focal=focal)
    quad = place_quad(true, 10.0, 23.1, 7.1, 40.9, 8.9)
    arrays, mats = assemble([(WALL, box((-3, -2, -12), (3, 2, 1)) + [quad]), (LAMP, [rect((0.0, 1.5, -9.0), (0.5, 0, 0), (0, 0, 0.5), (0, -1, 0))])])
    cam = axis_camera((0, 0, 0), w, h, focal=focal, right=(-1, 0, eps_right), up=(0, 1, eps_up))
    return Case("C4 telephoto, %s" % name, arrays, mats, cam, frames=(2, 7), gate=0, quad_pair=6)


def telephotos():
    e = 9e-5
    return [telephoto(e, 0, "right +"), telephoto(-e, 0, "right -"), telephoto(0, e, "up +"), telephoto(0, -e, "up -")]


def skewed():
    """C5: right off by 2e-4: the gate is 0"""
    arrays, mats = room()
    cam = axis_camera((0.1, 0.0, 1.0), W, H, right=(-1, 0, 2e-4))
    return Case("C5 basis off by 2e-4", arrays, mats, cam, gate=0)


def limit_skew(kind, sign):
    """C7: the cull ON next to the gate's limit.  f / sensor_x = 60 at 44 x 20 and a skew of 8.9e-5 -- under the 1e-4 of every Gram term
    -- give a worst-case shift of 0.24 of the 0.25 pixels the gate allows.  "forward": right = (-1, 0, 0) -+ eps forward, a quad whose
    TRUE projection (placed along the skewed basis' own rays) reaches 0.3 pixels into the tiles around it, where the frames' samples
    are.  "up": up = (0, 1, 0) +- eps right, and the quad's corners are 5 focal lengths above and below the axis (79 degrees off it), where
    the transposed projection of those corners is 5 x 0.24 pixels off in x (outwards for a quad that straddles the axis: a bound is a
    minimum or maximum over the corners): what the other seven eighths of the pad are for."""
    w, h = 44, 20
    focal = 60 * 0.036
    eps = sign * 0.24 / (w * (60 + 1.5 + 0.036 * (1 + h / w) / (4 * focal)))
    if kind == "forward":
        cam = axis_camera((0, 0, 0), w, h, focal=focal, right=(-1, 0, eps))
        quad = place_quad(cam, 10.0, 16 - 0.3, 8 - 0.3, 32 + 0.3, 16 + 0.3)
    else:
        cam = axis_camera((0, 0, 0), w, h, focal=focal, up=(-eps, 1, 0))
        tall = (5 * focal / float(cam.sy) + 0.5) * h  # the pixel row 5 focal lengths off the axis
        quad = place_quad(cam, 1.0, 16 - 0.3, h - tall, 32 + 0.3, tall)
    arrays, mats = assemble([(WALL, box((-3, -6, -12), (3, 6, 1)) + [quad]), (LAMP, [rect((0.0, 5.0, -9.0), (0.5, 0, 0), (0, 0, 0.5), (0, -1, 0))])])
    return Case("C7 skew at the limit, right.%s %s" % (kind, "+" if sign > 0 else "-"), arrays, mats, cam, frames=(2, 7), gate=1, quad_pair=6)


def pair_counts():
    """C6: 32 pairs (64 triangles); one pair plus loose triangles; no pair at all"""
    lo, hi = np.float64(BOX_LO), np.float64(BOX_HI)
    c, e = (lo + hi) / 2, (hi - lo) / 2
    X, Y, Z = np.diag(e)
    many = (grid(c - Y, X, Z, 3, 3, (0, 1, 0)) + grid(c + Y, X, -Z, 3, 3, (0, -1, 0)) + grid(c - Z, X, Y, 2, 2, (0, 0, 1)) +
            grid(c + Z, -X, Y, 2, 1, (0, 0, -1)) + grid(c - X, Z, Y, 2, 1, (1, 0, 0)) + grid(c + X, -Z, Y, 2, 1, (-1, 0, 0)) +
            inner_quads() + [rect((-0.4, 0.2, -0.6), (0.2, 0, 0), (0, 0.2, 0), (0, 0, 1))])
    lamp = lamp_quad((0.3, 0.9, -0.2), 0.25)
    cam = axis_camera((0.1, 0.0, 1.1), W, H, focal=0.025)
    out = [Case("C6 32 pairs", *assemble([(WALL, many), (LAMP, [lamp])]), cam, gate=1, pairs=32, singles=0)]
    loose = [("split",) + f[1:] for f in box(BOX_LO, BOX_HI, skip=("floor",)) + inner_quads()]
    floor = box(BOX_LO, BOX_HI)[0]
    out.append(Case("C6 one pair", *assemble([(WALL, [floor] + loose), (LAMP, [("split",) + lamp[1:]])]), cam, gate=1, pairs=1, singles=16))
    out.append(Case("C6 no pair", *assemble([(WALL, [("split",) + floor[1:]] + loose), (LAMP, [("split",) + lamp[1:]])]), cam, gate=1,
                    pairs=0, singles=18))
    return out


def tie_scene():
    """two halves of the ceiling, mirror images in x: with the light of frame 0 (x component exactly 0) their probe scores are bit-equal,
    and no pair's is higher -- the rank tie-break of lds_pscore / lds_score decides which one is probed first"""
    lo, hi = np.float64(BOX_LO), np.float64(BOX_HI)
    c, e = (lo + hi) / 2, (hi - lo) / 2
    X, Y, Z = np.diag(e)
    walls = grid(c + Y, X, -Z, 2, 1, (0, -1, 0)) + box(BOX_LO, BOX_HI, skip=("ceiling", "front")) + inner_quads()
    arrays, mats = assemble([(WALL, walls)])
    return Case("P ceiling halves tie", arrays, None, axis_camera((0.1, 0.0, 3.0), W, H), tied=(0, 1))


def open_top():
    """the open-top scene of tests/test_edge_cases_gpu.py at 64 x 48"""
    import test_edge_cases_gpu as T
    cam = T._ring_camera(64, 48)
    return Case("P open top", T._open_top_scene(), None, Cam(cam.position, cam.forward, cam.right, cam.up, cam.focal_length, cam.sensor_size[0], 64, 48))


# Every case by name.  Nothing is built until a test asks for it: `case(name)` builds once per process.
_BUILD = {}
for _s in (0.01, 0.1, 1.0, 10.0, 30.0):
    _BUILD["N1 cornell x%g" % _s] = functools.partial(cornell, _s)
for _f in (1.0 - 1e-3, 1.0 + 1e-3, 2.0):
    _BUILD["N2 lamp %.4g delta below the ceiling" % _f] = functools.partial(hanging, _f)
for _s in (0.0, 0.5, 0.99, 1.01, 2.0):
    _BUILD["N3 decal %.4g e-6 D outside" % _s] = functools.partial(decal, _s)
for _f in (0.5, 0.9, 1.1):
    _BUILD["N3 decal %.4g tolerances outside" % _f] = functools.partial(decal, None, _f)
_BUILD["N4 corridor"] = corridor
_BUILD["N5 kept reasons"] = kept_reasons
NEE_NAMES = list(_BUILD)
REFIT_NAMES = ["N6 lamp 8 delta below the ceiling", "N6 lamp 0.5 delta below the ceiling"]
_BUILD[REFIT_NAMES[0]] = functools.partial(hanging, 8.0, "N6")
_BUILD[REFIT_NAMES[1]] = functools.partial(hanging, 0.5, "N6")


def _register(names, builder):
    made = functools.lru_cache(None)(builder)
    for k, name in enumerate(names):
        _BUILD[name] = functools.partial(lambda k: made()[k], k)
    return names


CAMERA_NAMES = (_register(["C1 view %d at %dx%d" % (k, w, h) for k in range(8) for w, h in ((44, 20), (72, 40))], room_views) +
                _register(["C2 side walls straddle the camera plane", "C2 vertex one ulp below z = 1e-4", "C2 vertex one ulp above z = 1e-4",
                           "C2 facing a wall 2e-4 away", "C2 oblique to a wall 2e-4 away"], plane_cuts) +
                _register(["C3 edges %+.1f px, %s" % (off, n) for off in (-2.5, -1.5, -0.5, 0.5) for n in ("inner tiles", "last column and row")],
                          tile_edges) +
                _register(["C4 telephoto, %s" % n for n in ("right +", "right -", "up +", "up -")], telephotos) +
                _register(["C5 basis off by 2e-4"], lambda: [skewed()]) +
                _register(["C6 32 pairs", "C6 one pair", "C6 no pair"], pair_counts) +
                _register(["C7 skew at the limit, right.%s %s" % (k, sg) for k in ("forward", "up") for sg in "+-"],
                          lambda: [limit_skew(k, sg) for k in ("forward", "up") for sg in (1, -1)]))
_BUILD["P ceiling halves tie"] = tie_scene
_BUILD["P open top"] = open_top
# (case, EXT model): the C6 scenes in both models (CAP_NO_INLINE_NEE is the EXT model's switch), the tie and the open top
PROBE_NAMES = ([(n, False) for n in CAMERA_NAMES if n.startswith("C6")] + [(n, True) for n in CAMERA_NAMES if n.startswith("C6")] +
               [("P ceiling halves tie", False), ("P open top", False)])


@functools.lru_cache(None)
def case(name):
    c = _BUILD[name]()
    assert c.name == name, (c.name, name)
    return c


def cases(names, prefix=""):
    return [case(n) for n in names if n.startswith(prefix)]


# ------------------------------------------------------------------------------------------------
# the oracle's frames, computed once per (case, model, frame) and shared by the tests of a process
# ------------------------------------------------------------------------------------------------
DEPTH = 3
_REF = {}


def reference(case, ext, frame, bluenoise):
    key = (case.name, bool(ext), frame)
    if key not in _REF:
        from oracle import cap_oracle as O
        sc = O.Scene(*case.arrays, materials=case.mats) if ext else O.Scene(*case.arrays)
        _REF[key] = sc.render_frame(case.cam.oracle(), bluenoise, case.cam.w, case.cam.h, frame, DEPTH, flags=O.FLAG_EXT_MATERIALS if ext else 0,
                                    threads=8)
    return _REF[key]
