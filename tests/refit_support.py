"""Helpers of tests/test_refit_gpu.py: scenes as GeometryStorage arrays, deformations, the oracle's triangle test over candidate
triangles, the binary tree metric in numpy, and the dequantised boxes of the 8-wide view."""
import os
import sys

import numpy as np

from capsaicin_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
MISS = capi.MISS


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Scene:
    """positions / normals [V, 3], texcoords [V, 2] float32, indices [I] uint32, meshes [M, 8] uint32."""

    def __init__(self, positions, normals, texcoords, indices, meshes):
        self.positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self.texcoords = np.ascontiguousarray(texcoords, np.float32).reshape(-1, 2)
        self.indices = np.ascontiguousarray(indices, np.uint32).ravel()
        self.meshes = np.ascontiguousarray(meshes, np.uint32).reshape(-1, 8)

    def moved(self, positions=None, normals=None, texcoords=None):
        return Scene(self.positions if positions is None else positions, self.normals if normals is None else normals,
                     self.texcoords if texcoords is None else texcoords, self.indices, self.meshes)

    def vertex_mesh(self):
        """mesh index per vertex"""
        out = np.zeros(len(self.positions), np.int64)
        for m, d in enumerate(self.meshes):
            out[int(d[1]):int(d[1]) + int(d[0])] = m
        return out

    def triangles(self, positions=None):
        """(T, 3, 3) float32 vertices in global triangle order"""
        P = self.positions if positions is None else np.asarray(positions, np.float32).reshape(-1, 3)
        out = []
        for d in self.meshes:
            nv, fv, ni, fi = (int(x) for x in d[:4])
            out.append(P[self.indices[fi:fi + (ni // 3) * 3].astype(np.int64) + fv].reshape(-1, 3, 3))
        return np.concatenate(out).astype(np.float32)


def cornell_scene(cornell_path):
    g = capi.Geometry(cornell_path)
    return Scene(g.positions, g.normals, g.texcoords, g.indices, g.meshes), g.materials()


def hall_scene(scale=1.0):
    import make_sponza_class as gen
    P, N, T, I, D, _ = gen.arrays(scale, tex_size=128)
    return Scene(P, N, T, I, D)


def context(scene, build=None, bluenoise=None, materials=None, host_collapse=False):
    r = capi.Renderer(0)
    if build is not None:
        r.set_bvh_build(build)
    if host_collapse:
        r.debug_switch("CAP_WIDE_HOST_COLLAPSE", 1)
    r.upload_scene(scene.positions, scene.normals, scene.texcoords, scene.indices, scene.meshes)
    if bluenoise is not None:
        r.upload_bluenoise(bluenoise)
    if materials is not None:
        r.upload_materials(materials)
    r.build_bvh()
    return r


def trees(r):
    """(binary nodes as uint32, leaf order, wide nodes, wide tri_src, wide depth, top) of a context"""
    nodes, leaves = r.bvh_readback()
    wn, src, depth, top = r.bvh_wide_readback()
    return bits(nodes), leaves.copy(), wn.copy(), src.copy(), depth, top


def assert_same_trees(a, b, what=""):
    for k, name in enumerate(("binary nodes", "leaf order", "wide nodes", "wide tri_src", "wide depth", "wide top")):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "%s differ %s" % (name, what)


def half_area(lo, hi):
    d = hi - lo
    return d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]


def expected_node_visits(nodes):
    """1 + sum(inner child box area) / root box area over the binary readback, in float64"""
    if len(nodes) == 0:
        return 1.0
    bn = nodes.astype(np.float64)
    kid = nodes[:, 12:14].copy().view(np.int32)
    a0, a1 = half_area(bn[:, 0:3], bn[:, 3:6]), half_area(bn[:, 6:9], bn[:, 9:12])
    root = half_area(np.minimum(bn[:1, 0:3], bn[:1, 6:9]), np.maximum(bn[:1, 3:6], bn[:1, 9:12]))[0]
    return 1.0 + (a0[kid[:, 0] >= 0].sum() + a1[kid[:, 1] >= 0].sum()) / root


def padded_boxes(tris):
    """triangle boxes with the builders' leaf padding, float32 arithmetic"""
    lo, hi = tris.min(1), tris.max(1)
    pad = np.float32(1e-5) * np.maximum(np.float32(1.0), np.maximum(np.abs(lo), np.abs(hi)))
    return lo - pad, hi + pad


def check_binary_conservative(nodes, leaves, tris):
    """every binary child box contains its subtree's padded triangle boxes (children before parents by a post-order walk)"""
    f = nodes.view(np.float32) if nodes.dtype == np.uint32 else nodes
    kid = f[:, 12:14].copy().view(np.int32)
    plo, phi = padded_boxes(tris)
    n_inner = len(f)
    sub_lo, sub_hi = np.zeros((n_inner, 3), np.float32), np.zeros((n_inner, 3), np.float32)
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        stack.extend(int(c) for c in kid[i] if c >= 0)
    for i in reversed(order):
        los, his = [], []
        for s in range(2):
            c = int(kid[i, s])
            lo, hi = (sub_lo[c], sub_hi[c]) if c >= 0 else (plo[leaves[~c]], phi[leaves[~c]])
            box_lo, box_hi = f[i, 6 * s:6 * s + 3], f[i, 6 * s + 3:6 * s + 6]
            assert np.all(box_lo <= lo) and np.all(box_hi >= hi), "binary node %d slot %d is not conservative" % (i, s)
            los.append(lo), his.append(hi)
        sub_lo[i], sub_hi[i] = np.minimum(*los), np.maximum(*his)


def check_wide_conservative(wn, src, leaves, tris):
    """every dequantised wide child box contains the boxes of the triangles below it"""
    w = wn.astype(np.uint32)
    p = w[:, 0:3].view(np.float32).astype(np.float64)
    stp = np.stack([w[:, 3], w[:, 7] & np.uint32(0xffff0000), (w[:, 7] << np.uint32(16))], 1).view(np.float32).astype(np.float64)
    lo_t, hi_t = tris.min(1).astype(np.float64), tris.max(1).astype(np.float64)
    sub = {}

    def below(i):  # global triangle ids below wide node i
        if i in sub:
            return sub[i]
        out = []
        cb, tb, tv, im = int(w[i, 4]), int(w[i, 5]), int(w[i, 6]) & 0xffffff, int(w[i, 6]) >> 24
        for s in range(8):
            out.append(slot_tris(i, s, cb, tb, tv, im))
        sub[i] = out
        return out

    def slot_tris(i, s, cb, tb, tv, im):
        if im >> s & 1:
            c = cb + bin(im & ((1 << s) - 1)).count("1")
            return [g for lst in below(c) for g in lst]
        out = []
        for k in range(3):
            b = k * 8 + s
            if tv >> b & 1:
                out.append(int(leaves[src[tb + bin(tv & ((1 << b) - 1)).count("1")]]))
        return out

    for i in range(len(w) - 1, -1, -1):
        for s, gs in enumerate(below(i)):
            if not gs:
                continue
            q = [(int(w[i, 8 + 2 * a + (s >> 2)]) >> (8 * (s & 3))) & 0xff for a in range(6)]
            blo = p[i] + np.array(q[0:3], np.float64) * stp[i]
            bhi = p[i] + np.array(q[3:6], np.float64) * stp[i]
            assert np.all(blo <= lo_t[gs].min(0)) and np.all(bhi >= hi_t[gs].max(0)), "wide node %d slot %d is not conservative" % (i, s)


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
    """Per ray, the triangles whose float64 intersection lies within a relative margin of the nearest such t (torch float64 on the GPU)"""
    import torch
    dev = torch.device("cuda", 0)
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
        near = torch.isfinite(t) & (t <= (best + margin * (1.0 + best.abs()))[:, None])
        ri, ti = torch.nonzero(near, as_tuple=True)
        for a, b in zip(ri.tolist(), (ti + k * chunk).tolist()):
            out[a].append(b)
    return out


def check_brute_force(rays, recs, tris, all_triangles=False):
    """every record equals the oracle's winner over every triangle (all_triangles) or over the float64 candidates + the GPU's pick"""
    cands = None if all_triangles else candidates(rays, tris)
    bad = []
    for i in range(len(rays)):
        g = int(bits(recs[i])[3])
        c = range(len(tris)) if all_triangles else cands[i] + ([g] if g != MISS else [])
        want = exact(rays[i], tris, c)
        if not np.array_equal(bits(want), bits(recs[i])):
            bad.append((i, bits(recs[i]).tolist(), bits(want).tolist()))
    assert not bad, "%d of %d records differ, first: %s" % (len(bad), len(rays), bad[:3])


def rays_into(tris, rng, n, spread=0.3):
    """rays from points around the scene towards random triangles' interiors, plus random directions"""
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    c, ext = (lo + hi) / 2, (hi - lo)
    o = c + (rng.random((n, 3)) - 0.5) * ext * (1.0 + spread)
    g = rng.integers(0, len(tris), n)
    b = rng.dirichlet((1, 1, 1), n)
    target = np.einsum("nk,nkj->nj", b, tris[g].astype(np.float64))
    d = target - o
    d[: n // 4] = rng.normal(size=(n // 4, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, 0.0, d, np.inf
    r[n // 2:, 7] = 3.0  # bounded rays too
    return r


def hall_camera(w, h):
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


PLANES = (capi.BUF_GBUFFER_GEO, capi.BUF_DIRECT, capi.BUF_ALBEDO, capi.BUF_NORMAL_DEPTH, capi.BUF_INDIRECT, capi.BUF_ACCUM_SUM)


def render_result(r, cam, w, h, frames, depth, flags=capi.RENDER_AOV, batch_paths=None):
    r.set_resolution(w, h)
    r.set_camera(cam)
    if batch_paths:
        r.set_batch_paths(batch_paths)
    r.accum_reset()
    r.stats_reset()
    r.render(0, frames, depth, flags)
    r.sync()
    s = r.stats()
    out = {k: bits(r.readback(k)) for k in PLANES}
    out["rays"] = (s.rays_primary, s.rays_extension, s.rays_shadow, s.rays_extension_bounce0, s.rays_shadow_bounce0, s.shaded_vertices)
    return out


def assert_same_render(a, b, what=""):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "render plane %s differs %s" % (k, what)
