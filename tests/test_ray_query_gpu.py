"""Ray queries of caller-supplied rays (cap_trace_rays / cap_trace_occlusion) on the MI355X.  Every record is compared on its raw
uint32 bits: against the oracle's triangle test over every triangle (Cornell box), against the oracle's test on the candidates of
a float64 pass (262 k hall), against the render's own G-buffer, between the wide kernels and the binary-tree fallback and across
every builder; plus the argument contract and that a query leaves a render's results untouched."""
import ctypes
import os
import sys

import numpy as np
import pytest

from capsaicin_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
MISS = capi.MISS
SENTINEL = 0x7FBADBAD  # a NaN no record can hold


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def torch_dev():
    import torch
    return torch.device("cuda", 0)


def triangles(geo):
    """(T, 3, 3) float32 vertices in global triangle order: mesh-table order, then primitive order."""
    P = geo.positions.reshape(-1, 3)
    out = []
    for m in geo.meshes:
        nv, fv, ni, fi = (int(x) for x in m[:4])
        idx = geo.indices[fi:fi + (ni // 3) * 3].astype(np.int64) + fv
        out.append(P[idx].reshape(-1, 3, 3))
    return np.concatenate(out).astype(np.float32)


def exact(ray, tris, cands):
    """Record of the intersection contract over the candidate triangles, by the oracle's triangle test: min t, ties to the lower id."""
    from oracle import cap_oracle as O
    o, d = ray[0:3], ray[4:7]
    best_t, best_u, best_v, best_g = np.float32(ray[7]), np.float32(0), np.float32(0), MISS
    for g in sorted(set(int(c) for c in cands)):
        h = O.intersect_triangle(o, d, float(ray[3]), float(ray[7]), tris[g, 0], tris[g, 1], tris[g, 2])
        if h is None:
            continue
        t = np.float32(h[0])
        if t < best_t or (t == best_t and g < best_g):
            best_t, best_u, best_v, best_g = t, np.float32(h[1]), np.float32(h[2]), g
    rec = np.array([best_t, best_u, best_v, 0], np.float32)
    rec.view(np.uint32)[3] = best_g
    return rec


def candidates(rays, tris, margin=1e-4, chunk=8192):
    """Per ray, the triangles whose float64 intersection (with a relative margin on the barycentrics and the interval) lies within
    the margin of the nearest such t -- the only ones the float32 contract can pick (torch float64 on the GPU, chunked)."""
    import torch
    dev = torch_dev()
    R = torch.as_tensor(np.ascontiguousarray(rays, np.float32), device=dev).double()
    o, tmin, d, tmax = R[:, 0:3], R[:, 3], R[:, 4:7], R[:, 7]
    T = torch.as_tensor(tris, device=dev).double()
    best = torch.full((len(rays),), float("inf"), dtype=torch.float64, device=dev)
    hits = []
    for s in range(0, len(tris), chunk):
        v0, e1, e2 = T[s:s + chunk, 0], T[s:s + chunk, 1] - T[s:s + chunk, 0], T[s:s + chunk, 2] - T[s:s + chunk, 0]
        p = torch.cross(d[:, None, :].expand(-1, len(v0), -1), e2[None].expand(len(R), -1, -1), dim=2)
        det = (e1[None] * p).sum(2)
        tv = o[:, None, :] - v0[None]
        u = (tv * p).sum(2) / det
        q = torch.cross(tv, e1[None].expand(len(R), -1, -1), dim=2)
        v = (d[:, None, :] * q).sum(2) / det
        t = (e2[None] * q).sum(2) / det
        tol = margin * (1.0 + t.abs())
        ok = (u >= -margin) & (v >= -margin) & (u + v <= 1 + margin) & (t > tmin[:, None] - tol) & (t < tmax[:, None] + tol) & (det != 0)
        t = torch.where(ok, t, torch.full_like(t, float("inf")))
        best = torch.minimum(best, t.min(1).values)
        hits.append(t)
    out = [[] for _ in range(len(rays))]
    for k, t in enumerate(hits):
        near = torch.isfinite(t) & (t <= (best + margin * (1.0 + best.abs()))[:, None])  # (a ray that meets nothing has none)
        ri, ti = torch.nonzero(near, as_tuple=True)
        for a, b in zip(ri.tolist(), (ti + k * chunk).tolist()):
            out[a].append(b)
    return out


def check_against_candidates(rays, recs, tris):
    """Every GPU record equals the exact winner among the float64 candidates plus the triangle the GPU named."""
    cands = candidates(rays, tris)
    bad = []
    for i in range(len(rays)):
        g = int(bits(recs[i])[3])
        c = cands[i] + ([g] if g != MISS else [])
        want = exact(rays[i], tris, c)
        if not np.array_equal(bits(want), bits(recs[i])):
            bad.append((i, rays[i].tolist(), bits(recs[i]).tolist(), bits(want).tolist()))
    assert not bad, "%d of %d records differ, first: %s" % (len(bad), len(rays), bad[:3])


def rand_dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def ray_array(o, tmin, d, tmax):
    n = len(o)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


def renderer(geo, build=None, textures=()):
    r = capi.Renderer(0)
    if build is not None:
        r.set_bvh_build(build)
    r.upload_geometry(geo)
    for i, t in enumerate(textures):
        r.upload_texture(i, t)
    r.build_bvh()
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes and ray sets
@pytest.fixture(scope="module")
def cornell(cornell_path):
    geo = capi.Geometry(cornell_path)
    return geo, triangles(geo)


@pytest.fixture(scope="module")
def hall(tmp_path_factory):
    import make_sponza_class as gen
    d = str(tmp_path_factory.mktemp("hall"))
    gen.write(d, 1.0, 64)
    geo = capi.Geometry(os.path.join(d, "sponza_class.obj"))
    assert geo.indices.size // 3 > 250000
    return geo, triangles(geo), d


def degenerate_rays():
    nan, inf = np.float32("nan"), np.float32("inf")
    base = np.array([0.1, 1.0, 0.2, 0.0, 0.3, -0.4, 0.5, 10.0], np.float32)
    out = []
    for k in range(8):  # NaN in every component
        r = base.copy()
        r[k] = nan
        out.append(r)
    for k in (0, 1, 2, 4, 5, 6):  # infinite origin / direction components
        r = base.copy()
        r[k] = inf
        out.append(r)
    r = base.copy()
    r[4:7] = 0.0  # zero direction
    out.append(r)
    r = base.copy()
    r[4:7] = -0.0
    out.append(r)
    for tmin, tmax in ((1.0, 1.0), (2.0, 1.0), (0.0, 0.0), (0.0, -1.0), (inf, inf), (-inf, -inf)):
        r = base.copy()
        r[3], r[7] = tmin, tmax
        out.append(r)
    return np.array(out, np.float32)


@pytest.fixture(scope="module")
def cornell_rays(cornell):
    """~8 k rays: inside and outside the box (some far beyond the wide view's error budget), aimed at shared edges and vertices,
    leaving surfaces with tmin = 0 and a small tmin, tmax exactly at a hit's t, +inf tmax, and the degenerate rays."""
    geo, tris = cornell
    rng = np.random.default_rng(7)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    sets = []
    o = rng.uniform(lo + 0.02, hi - 0.02, (2500, 3))  # inside
    sets.append(ray_array(o, 0.0, rand_dirs(rng, 2500) * rng.uniform(0.5, 2.0, (2500, 1)), np.where(rng.random(2500) < 0.5, np.inf, 100.0)))
    c = (lo + hi) / 2
    for radius, n in ((4.0, 1200), (60.0, 200)):  # outside (60: beyond 4 x the scene size, the binary tree answers)
        o = c + rand_dirs(rng, n) * radius
        tgt = rng.uniform(lo, hi, (n, 3))
        sets.append(ray_array(o, 0.0, tgt - o, np.inf))
    # shared edges and vertices: targets at every vertex and edge midpoint (fan pairs share v0 and the v0 -> v2 edge)
    pts = np.concatenate([tris.reshape(-1, 3), (tris[:, 0] + tris[:, 1]) / 2, (tris[:, 1] + tris[:, 2]) / 2, (tris[:, 0] + tris[:, 2]) / 2])
    pts = pts.astype(np.float32)
    for reps in range(8):
        o = rng.uniform(lo + 0.05, hi - 0.05, (len(pts), 3)).astype(np.float32)
        sets.append(ray_array(o, 0.0, pts - o, np.inf))
    # on a surface: origin at a point of a triangle, tmin 0 and a small tmin, both sides
    n = 1000
    k = rng.integers(0, len(tris), n)
    b = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    o = (tris[k] * b[:, :, None]).sum(1).astype(np.float32)
    for tmin in (0.0, 1e-4):
        sets.append(ray_array(o, tmin, rand_dirs(rng, n), np.inf))
    rays = np.concatenate(sets).astype(np.float32)
    return rays, degenerate_rays()


@pytest.fixture(scope="module")
def cornell_expected(cornell, cornell_rays):
    geo, tris = cornell
    rays, _ = cornell_rays
    allc = range(len(tris))
    want = np.array([exact(r, tris, allc) for r in rays], np.float32)
    # tmax exactly at a hit's t: that hit must be rejected
    hit = np.nonzero(bits(want)[:, 3] != MISS)[0][:600]
    extra = rays[hit].copy()
    extra[:, 7] = want[hit, 0]
    want_extra = np.array([exact(r, tris, allc) for r in extra], np.float32)
    assert np.all(bits(want_extra)[:, 3] != bits(want[hit])[:, 3])
    rays = np.concatenate([rays, extra])
    want = np.concatenate([want, want_extra])
    assert len(rays) >= 8000
    return rays, want


def hall_rays(r, geo, tris, n_random=1024, n_hemi=512, seed=3):
    """Random rays inside the hall's box, cosine-hemisphere rays from camera hits, and a few from far outside."""
    import make_sponza_class as gen
    from oracle import cap_oracle as O
    rng = np.random.default_rng(seed)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    o = rng.uniform(lo + 0.01, hi - 0.01, (n_random, 3))
    sets = [ray_array(o, 0.0, rand_dirs(rng, n_random), np.inf)]
    c = gen.camera()
    cam = O.make_camera(tuple(c["position"]), tuple(c["forward"]), tuple(-np.cross(c["forward"], (0, 1, 0))), (0, 1, 0), 0.036, 0.024,
                        c["focal_length"])
    cam_rays = []
    for _ in range(n_hemi):
        co, cd = O.primary_ray(cam, int(rng.integers(0, 96)), int(rng.integers(0, 64)), 96, 64, 0)
        cam_rays.append(np.concatenate([co, [0.0], cd, [1e6]]))
    cam_rays = np.array(cam_rays, np.float32)
    h = r.trace_rays(cam_rays)
    ok = bits(h)[:, 3] != MISS
    cr, h = cam_rays[ok], h[ok]
    g = bits(h)[:, 3].astype(np.int64)
    p = (cr[:, 0:3] + h[:, 0:1] * cr[:, 4:7]).astype(np.float32)
    nrm = np.cross(tris[g, 1] - tris[g, 0], tris[g, 2] - tris[g, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= -np.sign((nrm * cr[:, 4:7]).sum(1, keepdims=True))  # facing the camera
    s = [O.map_to_hemisphere(rng.random(2), n) for n in nrm]
    sets.append(ray_array(p, 1e-4, np.array(s), np.inf))
    far = (lo + hi) / 2 + rand_dirs(rng, 64) * 500.0
    sets.append(ray_array(far, 0.0, rng.uniform(lo, hi, (64, 3)) - far, np.inf))
    return np.concatenate(sets).astype(np.float32)


@pytest.fixture(scope="module")
def hall_ctx(hall):
    geo, tris, _ = hall
    r = renderer(geo)
    assert r.debug_get(capi.Renderer.DEBUG_WIDE_IN_USE) == 1
    rays = hall_rays(r, geo, tris)
    yield r, rays
    r.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. Cornell box against the brute force
def test_cornell_brute_force(native_lib, cornell, cornell_rays, cornell_expected):
    geo, tris = cornell
    rays, want = cornell_expected
    r = renderer(geo)
    assert r.debug_get(capi.Renderer.DEBUG_WIDE_IN_USE) == 1
    got = r.trace_rays(rays)
    bad = np.nonzero((bits(got) != bits(want)).any(1))[0]
    assert len(bad) == 0, "%d of %d records differ, first %s: got %s want %s" % (len(bad), len(rays), rays[bad[0]], bits(got[bad[0]]), bits(want[bad[0]]))
    assert (bits(want)[:, 3] != MISS).mean() > 0.5
    # degenerate rays: exact miss records (tmax, 0, 0, ~0), occlusion 0
    deg = cornell_rays[1]
    got = r.trace_rays(deg)
    miss = np.zeros((len(deg), 4), np.float32)
    miss[:, 0] = deg[:, 7]
    miss.view(np.uint32)[:, 3] = MISS
    assert np.array_equal(bits(got), bits(miss))
    assert np.array_equal(r.trace_occlusion(deg), np.zeros(len(deg), np.int32))
    r.close()


def test_cornell_tie_rule_is_exercised(cornell, cornell_expected):
    """The edge / vertex rays do meet equal-t hits on two triangles (the tie rule decides them)."""
    from oracle import cap_oracle as O
    geo, tris = cornell
    rays, want = cornell_expected
    ties = 0
    for i in range(0, len(rays), 3):
        g = int(bits(want[i])[3])
        if g == MISS:
            continue
        for k in range(len(tris)):
            if k != g:
                h = O.intersect_triangle(rays[i, 0:3], rays[i, 4:7], float(rays[i, 3]), float(rays[i, 7]), *tris[k])
                if h is not None and np.float32(h[0]) == want[i, 0]:
                    ties += 1
                    assert k > g
    assert ties > 20


# 2. the 262 k hall against the float64 candidates
def test_hall_against_candidates(native_lib, hall, hall_ctx):
    geo, tris, _ = hall
    r, rays = hall_ctx
    got = r.trace_rays(rays)
    assert (bits(got)[:, 3] != MISS).mean() > 0.5
    check_against_candidates(rays, got, tris)


# 3. camera rays reproduce the G-buffer
def _gbuffer_case(r, cam, w, h, fc):
    from oracle import cap_oracle as O
    r.set_resolution(w, h)
    r.set_camera(cam)
    r.render(fc, 1, 1, capi.RENDER_AOV)
    gb = r.readback(capi.BUF_GBUFFER_GEO)
    ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1],
                         cam.focal_length)
    rays = np.zeros((h * w, 8), np.float32)
    for y in range(h):
        for x in range(w):
            o, d = O.primary_ray(ocam, x, y, w, h, fc)
            rays[y * w + x] = (*cam.position, 0.0, *d, 1e6)
    got = r.trace_rays(rays)
    inst, prim = r.triangle_to_instance_primitive(capi.hit_triangles(got))
    g = bits(gb).reshape(-1, 4)
    assert np.array_equal(inst, g[:, 2].astype(np.int64)) and np.array_equal(prim, g[:, 3].astype(np.int64))
    hit = g[:, 2] != MISS
    assert hit.mean() > 0.5
    assert np.array_equal(bits(got)[hit, 1:3], g[hit, 0:2])  # (t, u, v, id) against (u, v, instance, primitive)


@pytest.mark.parametrize("fc", [0, 7])
def test_camera_rays_reproduce_gbuffer_cornell(native_lib, bluenoise, cornell, fc):
    geo, _ = cornell
    r = renderer(geo)
    r.upload_bluenoise(bluenoise)
    _gbuffer_case(r, capi.cornell_camera(100, 60), 100, 60, fc)
    r.close()


def _hall_camera(w, h):
    import make_sponza_class as gen
    c = gen.camera()
    cam = capi.CameraData()
    f = np.float64(c["forward"])
    f /= np.linalg.norm(f)
    right = -np.cross(f, (0, 1, 0))
    right /= np.linalg.norm(right)
    cam.position[:] = c["position"]
    cam.forward[:] = f
    cam.right[:] = right
    cam.up[:] = np.cross(f, right)
    cam.focal_length = c["focal_length"]
    cam.sensor_size[0] = 0.036
    cam.sensor_size[1] = np.float32(0.036) * (np.float32(h) / np.float32(w))
    return cam


@pytest.mark.parametrize("fc", [0, 7])
def test_camera_rays_reproduce_gbuffer_hall(native_lib, bluenoise, hall, hall_ctx, fc):
    r, _ = hall_ctx
    r.upload_bluenoise(bluenoise)
    _gbuffer_case(r, _hall_camera(100, 60), 100, 60, fc)


# 4. wide kernels, binary-tree fallback and every builder give the same bits; 5. occlusion semantics
def _both(r, rays):
    return bits(r.trace_rays(rays)), r.trace_occlusion(rays)


def test_paths_and_builders_agree_cornell(native_lib, cornell, cornell_expected):
    geo, tris = cornell
    rays, want = cornell_expected
    ref = None
    for build in (0, 1, 2, 3, 4):
        r = renderer(geo, build)
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            assert r.debug_get(capi.Renderer.DEBUG_WIDE_IN_USE) == 1 - no_wide
            got = _both(r, rays)
            assert np.array_equal(got[0], bits(want)), "builder %d no_wide8 %d" % (build, no_wide)
            if ref is None:
                ref = got
            assert np.array_equal(got[1], ref[1]), "occlusion: builder %d no_wide8 %d" % (build, no_wide)
        r.close()


def test_paths_and_builders_agree_hall(native_lib, hall, hall_ctx):
    geo, tris, _ = hall
    r0, rays = hall_ctx
    ref = _both(r0, rays)
    r0.debug_switch("CAP_NO_WIDE8", 1)
    try:
        assert r0.debug_get(capi.Renderer.DEBUG_WIDE_IN_USE) == 0
        got = _both(r0, rays)
    finally:
        r0.debug_switch("CAP_NO_WIDE8", None)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    for build in (1, 2, 3, 4):
        r = renderer(geo, build)
        got = _both(r, rays)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), "builder %d" % build
        r.close()


def _occlusion_semantics(r, rays):
    m = 1e-5
    closest = r.trace_rays(rays)
    occ = r.trace_occlusion(rays)
    assert occ.dtype == np.int32 and set(np.unique(occ)) <= {0, 1}
    t, g = closest[:, 0].astype(np.float64), bits(closest)[:, 3]
    tmin, tmax = rays[:, 3].astype(np.float64), rays[:, 7].astype(np.float64)
    with np.errstate(invalid="ignore"):  # (inf - inf of a miss with tmax = inf)
        inside = (g != MISS) & (t > tmin + m * (1 + np.abs(t))) & (t < tmax - m * (1 + np.abs(t)))
    assert np.all(occ[inside] == 1) and inside.sum() > len(rays) // 4
    wide = rays.copy()
    wide[:, 3] = (tmin - m * (1 + np.abs(tmin))).astype(np.float32)
    wide[:, 7] = np.where(np.isinf(tmax), tmax, tmax + m * (1 + np.abs(tmax))).astype(np.float32)
    none = bits(r.trace_rays(wide))[:, 3] == MISS
    assert np.all(occ[none] == 0) and none.sum() > 0


def test_occlusion_semantics_cornell(native_lib, cornell, cornell_expected):
    geo, _ = cornell
    rays, _ = cornell_expected
    r = renderer(geo)
    _occlusion_semantics(r, rays)
    r.close()


def test_occlusion_semantics_hall(native_lib, hall_ctx):
    r, rays = hall_ctx
    _occlusion_semantics(r, rays)


# 6. sizes, the sentinel behind the output, the argument contract
@pytest.mark.parametrize("n", [1, 63, 64, 65, (1 << 22) + 3])
def test_sizes_leave_the_rest_untouched(native_lib, hall, hall_ctx, n):
    import torch
    geo, tris, _ = hall
    r, base = hall_ctx
    dev = torch_dev()
    reps = (n + len(base) - 1) // len(base)
    rays = torch.as_tensor(np.tile(base, (reps, 1))[:n], device=dev).contiguous()
    buf = torch.full((n + 64, 4), 0, dtype=torch.int32, device=dev).fill_(SENTINEL).view(torch.float32)
    occ = torch.full((n + 64,), SENTINEL, dtype=torch.int32, device=dev)
    out = r.trace_rays(rays, out=buf[:n])
    o2 = r.trace_occlusion(rays, out=occ[:n])
    assert out.data_ptr() == buf.data_ptr() and o2.data_ptr() == occ.data_ptr()
    b = buf.view(torch.int32).cpu().numpy()
    assert np.all(b[n:] == SENTINEL) and np.all(occ.cpu().numpy()[n:] == SENTINEL)
    assert not np.any((b[:n] == SENTINEL).all(1)) and set(np.unique(occ.cpu().numpy()[:n])) <= {0, 1}
    recs = buf[:n].cpu().numpy()
    pick = np.unique(np.concatenate([np.arange(min(n, 65)), np.arange(max(0, n - 64), n),
                                     np.random.default_rng(n).integers(0, n, 128)]))
    check_against_candidates(np.tile(base, (reps, 1))[:n][pick], recs[pick], tris)
    # the same rays give the same records whatever the launch they are in
    once = bits(r.trace_rays(base))
    assert np.array_equal(bits(recs[pick]), once[pick % len(base)])


def test_one_triangle_scene(native_lib):
    r = capi.Renderer(0)
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    meshes = np.array([[3, 0, 3, 0, 0, 0xFFFFFFFF, 0, 0]], np.uint32)
    r.upload_scene(pos, np.tile([0, 0, 1], (3, 1)).astype(np.float32), np.zeros((3, 2), np.float32), np.arange(3, dtype=np.uint32), meshes)
    r.build_bvh()
    rng = np.random.default_rng(1)
    o = np.concatenate([rng.uniform(-0.2, 1.2, (200, 2)), rng.choice([-1.0, 1.0], (200, 1))], 1)
    rays = ray_array(o, 0.0, np.tile([0, 0, 1.0], (200, 1)) * -np.sign(o[:, 2:3]), np.inf)
    got = r.trace_rays(rays)
    want = np.array([exact(x, pos[None], [0]) for x in rays], np.float32)
    assert np.array_equal(bits(got), bits(want)) and 0 < (bits(got)[:, 3] == 0).sum() < 200
    for no_wide in (0, 1):
        r.debug_switch("CAP_NO_WIDE8", no_wide)
        assert np.array_equal(bits(r.trace_rays(rays)), bits(want))
        assert np.array_equal(r.trace_occlusion(rays), (bits(want)[:, 3] == 0).astype(np.int32))
    r.close()


def test_argument_contract(native_lib, cornell):
    import torch
    geo, _ = cornell
    dev = torch_dev()
    L = capi.lib()
    rays = torch.zeros((128, 8), dtype=torch.float32, device=dev)
    rays[:, 6] = 1.0
    rays[:, 7] = 10.0
    out = torch.full((130, 4), SENTINEL, dtype=torch.int32, device=dev)
    occ = torch.full((130,), SENTINEL, dtype=torch.int32, device=dev)
    R, O_, H = rays.data_ptr(), occ.data_ptr(), out.data_ptr()
    r = capi.Renderer(0)
    r.upload_geometry(geo)
    # before cap_bvh_build
    assert L.cap_trace_rays(r.ctx, R, 128, H, 0) == 3 and L.cap_trace_occlusion(r.ctx, R, 128, O_, 0) == 3
    with pytest.raises(capi.CapError, match="cap_bvh_build"):
        r.trace_rays(rays)
    r.build_bvh()
    for fn, dst in ((L.cap_trace_rays, H), (L.cap_trace_occlusion, O_)):
        assert fn(r.ctx, R, 128, dst, 1) == 1  # reserved flags
        assert fn(r.ctx, R, 128, dst, 0x80000000) == 1
        assert fn(r.ctx, None, 128, dst, 0) == 1 and fn(r.ctx, R, 128, None, 0) == 1  # NULL
        assert fn(r.ctx, R + 4, 64, dst, 0) == 1 and fn(r.ctx, R, 64, dst + 8, 0) == 1  # misaligned
        assert fn(r.ctx, R, 128, R + 32 * 64, 0) == 1 and fn(r.ctx, R + 256, 16, R + 256 + 16, 0) == 1  # overlapping
        assert fn(r.ctx, R + 256, 16, R + 256, 0) == 1 and fn(r.ctx, R + 256, 4, R + 256 + 96, 0) == 1
        assert fn(r.ctx, R, 0, dst, 0) == 0  # nothing to do
    assert fn(None, R, 1, H, 0) == 1
    r.sync()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL) and np.all(occ.cpu().numpy() == SENTINEL)  # nothing was written
    assert np.all(rays.cpu().numpy()[:, 7] == 10.0)
    # the binding's own checks
    with pytest.raises(capi.CapError):
        r.trace_rays(rays.double())
    with pytest.raises(capi.CapError):
        r.trace_rays(rays[:, :4])
    empty = r.trace_rays(torch.zeros((0, 8), dtype=torch.float32, device=dev))
    assert tuple(empty.shape) == (0, 4)
    r.close()


def test_sync_false_on_torch_stream(native_lib, cornell, cornell_expected):
    """A renderer created on torch's stream: sync=False only enqueues, torch's stream orders everything."""
    import torch
    geo, _ = cornell
    rays, want = cornell_expected
    dev = torch_dev()
    stream = torch.cuda.Stream(dev)  # (a stream of its own: the null stream's handle is 0, which cap_ctx_create reads as "make one")
    with torch.cuda.stream(stream):
        r = capi.Renderer(0, stream.cuda_stream)
        r.upload_geometry(geo)
        r.build_bvh()
        t = torch.as_tensor(rays, device=dev)
        h = r.trace_rays(t, sync=False)
        o = r.trace_occlusion(t, sync=False)
        assert np.array_equal(bits(h.cpu().numpy()), bits(want))
        assert tuple(o.shape) == (len(rays),) and o.dtype == torch.int32
        r.close()


# 7. a query leaves the render's results untouched
@pytest.mark.parametrize("feedback", [False, True])
def test_queries_do_not_interfere_with_rendering(native_lib, bluenoise, hall, hall_ctx, feedback):
    geo, tris, d = hall
    _, rays = hall_ctx
    w, h, D = 96, 64, 3
    cam = _hall_camera(w, h)
    gs = capi.PostSettings()

    def run(query):
        r = capi.Renderer(0)
        r.upload_geometry(geo)
        r.upload_bluenoise(bluenoise)
        r.build_bvh()
        r.set_resolution(w, h)
        r.set_camera(cam)
        r.set_prev_camera(cam)
        r.set_batch_paths(w * h)  # one frame per batch: the batches alternate between two lanes
        lanes = []

        def frames(f0):
            if feedback:
                for f in range(f0, f0 + 4):
                    r.render(f, 1, D, capi.RENDER_AOV | capi.RENDER_GBUFFER_FEEDBACK)
                    r.post_frame(gs, f, cam)
            else:
                r.render(f0, 4, D, capi.RENDER_AOV)
                lanes.append(r.debug_get(capi.Renderer.DEBUG_LANES_USED))

        frames(0)
        q = None
        if query:
            q = (bits(r.trace_rays(rays)), r.trace_occlusion(rays))
        frames(4)
        if not feedback:
            assert lanes == [2, 2]
            r.post_frame(gs, 7, cam)
        s = r.stats()
        out = {"accum": bits(r.readback(capi.BUF_ACCUM_SUM)), "post": bits(r.post_readback()),
               "stats": (s.rays_primary, s.rays_extension, s.rays_shadow, s.shaded_vertices, s.frames, s.rays_extension_bounce0,
                         s.rays_shadow_bounce0, s.shadow_entries, s.shadow_entries_bounce0, s.guard_shade, s.guard_trace_any,
                         s.guard_append, s.launches_trace_closest, s.launches_trace_any, s.launches_shade, s.post_frames)}
        for kind in (capi.BUF_GBUFFER_GEO, capi.BUF_DIRECT, capi.BUF_ALBEDO, capi.BUF_NORMAL_DEPTH, capi.BUF_INDIRECT):
            out[kind] = bits(r.readback(kind))
        r.close()
        return out, q

    a, q = run(True)
    b, _ = run(False)
    for k in b:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "differs after a query: %s" % (k,)
    assert b["stats"][0] == 8 * w * h
    # and the queries themselves answered as on their own context
    r0, _ = hall_ctx
    assert np.array_equal(q[0], bits(r0.trace_rays(rays))) and np.array_equal(q[1], r0.trace_occlusion(rays))
