"""Helpers of the instanced ray-query tests (cap_instances_set, cap_trace_instances*): the object-space ray of the contract in
single-rounded float32 operations, the box-free brute force every GPU record is compared with (the oracle's triangle test per
instance, merged in (t, instance, triangle) order), a float64 candidate prefilter that may only add candidates, and the generators of
meshes, transforms and rays."""
import numpy as np

from filter_support import MISS, all_hits, bits, f32, facing, fma, keep, occludes  # noqa: F401  (re-exported for the tests)


# ---- the contract's object-space ray ----
def _dot(a, b):  # fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))
    return fma(a[2], b[2], fma(a[1], b[1], f32(a[0]) * f32(b[0])))


def ray_ok(ray):
    """query_ray_ok: finite origin and direction, a direction that is not zero, tmin < tmax"""
    r = np.asarray(ray, f32)
    return bool(np.all(np.isfinite(r[[0, 1, 2, 4, 5, 6]])) and np.any(r[4:7] != 0) and r[7] > r[3])


def to_object(W, ray):
    """The object-space ray of `ray` under the stored world-to-object matrix W (3, 4) float32, every operation a single-rounded
    float32 one: o'_r = dot(W_r.xyz, o) + W_r.w, d'_r = dot(W_r.xyz, d); tmin, tmax unchanged.  None when it is degenerate."""
    W = np.asarray(W, f32).reshape(3, 4)
    r = np.asarray(ray, f32)
    with np.errstate(all="ignore"):
        o = [f32(_dot(W[k, :3], r[0:3]) + W[k, 3]) for k in range(3)]
        d = [_dot(W[k, :3], r[4:7]) for k in range(3)]
    out = np.array([o[0], o[1], o[2], r[3], d[0], d[1], d[2], r[7]], f32)
    return out if ray_ok(out) else None


def merge(per_instance):
    """[(i, [(t, u, v, g), ...]), ...] -> [(t, u, v, i, g), ...] in (t, i, g) order"""
    out = [(t, u, v, i, g) for i, hits in per_instance for (t, u, v, g) in hits]
    out.sort(key=lambda h: (h[0], h[3], h[4]))
    return out


def instanced_hits(ray, W, live, inst_masks, tris, mesh_of_tri=None, mesh_masks=None, cull=None, mask=None, cands=None):
    """The filtered hit set of one world ray in (t, i, g) order as (t, u, v, i, g).  W: (N, 3, 4) as read back; live: (N,) bool;
    inst_masks: (N,) or None (0xFF); cands: {instance: iterable of triangles} or None (everything)."""
    if not ray_ok(ray):
        return []
    per = []
    for i in (range(len(W)) if cands is None else sorted(cands)):
        if not live[i]:
            continue
        im = 0xFF if inst_masks is None else int(inst_masks[i])
        ro = to_object(W[i], ray)
        if ro is None:
            continue
        hits = []
        for (t, u, v, g) in all_hits(ro, tris, None if cands is None else cands[i]):
            mm = 0xFF if mesh_masks is None else int(mesh_masks[mesh_of_tri[g]])
            if keep(facing(ro, tris[g]), mm & im, cull, mask):
                hits.append((t, u, v, g))
        per.append((i, hits))
    return merge(per)


def instanced_occlusion(ray, W, live, inst_masks, tris, mesh_of_tri=None, mesh_masks=None, cull=None, mask=None, cands=None):
    """1 when some (instance, triangle) that passes the filters satisfies the occlusion form against the object-space ray"""
    if not ray_ok(ray):
        return 0
    for i in (range(len(W)) if cands is None else sorted(cands)):
        if not live[i]:
            continue
        im = 0xFF if inst_masks is None else int(inst_masks[i])
        ro = to_object(W[i], ray)
        if ro is None:
            continue
        for g in (range(len(tris)) if cands is None else sorted(set(int(c) for c in cands[i]))):
            mm = 0xFF if mesh_masks is None else int(mesh_masks[mesh_of_tri[g]])
            if keep(facing(ro, tris[g]), mm & im, cull, mask) and occludes(ro, tris[g]):
                return 1
    return 0


def closest_record(hits, tmax):
    """(CapHit as 4 uint32 words, instance) of a merged hit list: its first entry, or the miss record"""
    rec = np.zeros(4, f32)
    rec[0] = tmax
    rec.view(np.uint32)[3] = MISS
    inst = MISS
    if hits:
        t, u, v, i, g = hits[0]
        rec[0:3] = (t, u, v)
        rec.view(np.uint32)[3] = g
        inst = i
    return rec.view(np.uint32).copy(), inst


def candidates(rays, W, live, tris, chunk=64):
    """Per ray {instance: [triangles]}: every pair whose float64 intersection with the (float32-rounded, up to double rounding)
    object-space ray passes with a generous margin -- on the barycentrics 1e-3 plus 1e-5 per triangle size of distance, on the interval
    1e-4 relative -- plus every pair the ray is nearly edge-on to.  A superset of what the float32 contract can accept; only ever adds."""
    R = np.asarray(rays, f32).astype(np.float64)
    Wd = np.asarray(W, f32).astype(np.float64)
    T = np.asarray(tris, f32).astype(np.float64)
    v0, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    nrm = np.cross(e1, e2)
    emin = np.minimum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1))
    out = [dict() for _ in range(len(R))]
    lv = np.flatnonzero(live)
    with np.errstate(all="ignore"):
        for s in range(0, len(R), chunk):
            r = R[s:s + chunk]
            o = (np.einsum("ikl,rl->rik", Wd[lv][:, :, :3], r[:, 0:3]) + Wd[lv][None, :, :, 3]).astype(f32).astype(np.float64)
            d = np.einsum("ikl,rl->rik", Wd[lv][:, :, :3], r[:, 4:7]).astype(f32).astype(np.float64)
            tv = o[:, :, None, :] - v0[None, None]                       # (r, i, t, 3)
            dd = d[:, :, None, :]
            p = np.cross(dd, e2[None, None])
            det = (e1[None, None] * p).sum(-1)
            u = (tv * p).sum(-1) / det
            q = np.cross(tv, e1[None, None])
            v = (dd * q).sum(-1) / det
            t = (e2[None, None] * q).sum(-1) / det
            m = 1e-3 + 1e-5 * np.linalg.norm(tv, axis=-1) / emin[None, None]
            tol = 1e-4 * (1.0 + np.abs(t))
            ok = (u >= -m) & (v >= -m) & (u + v <= 1 + m) & (t > r[:, None, None, 3] - tol) & (t < r[:, None, None, 7] + tol)
            edge_on = np.abs(det) <= 1e-6 * np.linalg.norm(d, axis=-1)[:, :, None] * np.linalg.norm(nrm, axis=1)[None, None]
            ok = (ok | edge_on | ~np.isfinite(u) | ~np.isfinite(v) | ~np.isfinite(t)) & np.isfinite(o).all(-1)[:, :, None]
            for a, b, c in zip(*np.nonzero(ok)):
                out[s + a].setdefault(int(lv[b]), []).append(int(c))
    return out


def expected(rays, W, live, inst_masks, tris, mesh_of_tri=None, mesh_masks=None, cull=None, mask=None, cands=None):
    """(records (N, 4) uint32, instances (N,) uint32, occlusion (N,) int32, hit lists) of the brute force"""
    if cands is None:
        cands = candidates(rays, W, live, tris)
    rec, inst, occ, lists = [], [], [], []
    for ray, c in zip(rays, cands):
        h = instanced_hits(ray, W, live, inst_masks, tris, mesh_of_tri, mesh_masks, cull, mask, c)
        a, b = closest_record(h, ray[7])
        rec.append(a), inst.append(b), lists.append(h)
        occ.append(instanced_occlusion(ray, W, live, inst_masks, tris, mesh_of_tri, mesh_masks, cull, mask, c))
    return np.array(rec, np.uint32).reshape(-1, 4), np.array(inst, np.uint32), np.array(occ, np.int32), lists


# ---- generators ----
def unit_cube():
    """The cube [0, 1]^3, one mesh per face (6 meshes of 2 triangles, outward winding): its vertices are the corners of its own
    root box, so silhouette rays graze the instance box.  Returns (positions, normals, texcoords, indices, meshes), triangles."""
    faces = [((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)), ((0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)),
             ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)), ((0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)),
             ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)), ((1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1))]
    P, I, M = [], [], []
    for m, f in enumerate(faces):
        M.append([4, len(P), 6, len(I), m, 0xFFFFFFFF, 0, 0])
        P += list(f)
        I += [0, 1, 2, 0, 2, 3]
    P, I = np.array(P, f32), np.array(I, np.uint32)
    N, T = np.tile(f32([0, 0, 1]), (len(P), 1)), np.zeros((len(P), 2), f32)
    tris = np.stack([P[4 * (g // 2) + I[3 * g:3 * g + 3].astype(np.int64)] for g in range(12)])
    return (P, N, T, I, np.array(M, np.uint32)), tris.astype(f32)


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def regular_transforms(n, seed=5, spread=20.0):
    """n object-to-world matrices (n, 3, 4) float32 every one of which must be live: translations, rotations, uniform scales from
    1e-3 to 1e3, anisotropy and shear up to a 2-norm condition number of 100, mirrors (negative determinant); some share a place so
    that instances overlap."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = i % 6
        t = rng.uniform(-spread, spread, 3)
        if i % 7 == 3 and out:
            t = out[-1][:, 3] + rng.uniform(-0.3, 0.3, 3)  # on top of the previous instance
        if kind == 0:
            L = np.eye(3)
        elif kind == 1:
            L = rotation(rng)
        elif kind == 2:
            L = rotation(rng) * 10.0 ** rng.uniform(-3, 3)
        elif kind == 3:
            s = np.array([1.0, 10.0 ** rng.uniform(0, 1), 10.0 ** rng.uniform(1, 1.99)])
            L = rotation(rng) @ np.diag(s) @ rotation(rng) * 10.0 ** rng.uniform(-1, 0)
        elif kind == 4:
            L = np.eye(3)
            L[0, 1], L[1, 2] = rng.uniform(-4, 4), rng.uniform(-2, 2)
            L = rotation(rng) @ L
        else:
            L = rotation(rng) @ np.diag([-1.0, 1.0, 1.0]) * 10.0 ** rng.uniform(-1, 1)
        M = np.c_[L, t].astype(f32)
        assert np.linalg.cond(M[:, :3].astype(np.float64)) <= 100.0, (i, kind)
        out.append(M)
    return np.stack(out)


def extreme_transforms(seed=6):
    """(matrices (n, 3, 4) float32, must_be_inert (n,) bool): condition numbers 1e3 .. 1e6 (inert, or live and exact), one singular,
    one with a NaN, one with an infinity (inert)."""
    rng = np.random.default_rng(seed)
    out, inert = [], []
    for c in (1e3, 1e4, 1e5, 1e6):
        L = rotation(rng) @ np.diag([1.0, np.sqrt(c), c]) @ rotation(rng) / np.sqrt(c)
        out.append(np.c_[L, rng.uniform(-5, 5, 3)]), inert.append(False)
    S = rotation(rng)
    S[2] = S[0] * 2.0  # rank 2
    out.append(np.c_[S, [1, 2, 3]]), inert.append(True)
    out.append(np.c_[np.zeros((3, 3)), [0, 0, 0]]), inert.append(True)
    Nn = np.c_[np.eye(3), [0, 0, 0]]
    Nn[1, 1] = np.nan
    out.append(Nn), inert.append(True)
    In = np.c_[np.eye(3), [0, np.inf, 0]]
    out.append(In), inert.append(True)
    return np.stack(out).astype(f32), np.array(inert)


def _ray(o, d, tmin=0.0, tmax=np.inf):
    return np.array([*o, tmin, *d, tmax], f32)


def aimed_rays(M, lo, hi, per_instance=3, seed=9, distances=(1.0, 100.0, 10000.0)):
    """Rays at each instance's centre, transformed box corners and edge midpoints from 1, 100 and 10 000 object sizes away."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    pts = [0.5 * (lo + hi)]
    grid = [(a, b, c) for a in (0, 0.5, 1) for b in (0, 0.5, 1) for c in (0, 0.5, 1)]
    pts += [lo + np.array(g) * (hi - lo) for g in grid if sum(1 for x in g if x == 0.5) <= 1]  # 8 corners, 12 edge midpoints
    rays = []
    for A in np.asarray(M, np.float64):
        if not np.all(np.isfinite(A)):
            continue
        size = np.linalg.norm(A[:, :3] @ (hi - lo))
        for _ in range(per_instance):
            p = A[:, :3] @ pts[rng.integers(len(pts))] + A[:, 3]
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            dist = distances[rng.integers(len(distances))] * max(size, 1e-30)
            rays.append(_ray(p + u * dist, -u * rng.uniform(0.5, 2.0)))
    return np.array(rays, f32)


def random_rays(n, box=25.0, seed=10):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-box, box, (n, 3))
    d = rng.normal(size=(n, 3))
    tmin = np.where(rng.random(n) < 0.2, rng.uniform(0, 5, n), 0.0)
    tmax = np.where(rng.random(n) < 0.3, rng.uniform(5, 60, n), np.inf)
    return np.c_[o, tmin, d, tmax].astype(f32)


def degenerate_rays():
    return np.array([_ray((0, 0, 0), (0, 0, 0)), _ray((np.nan, 0, 0), (0, 0, 1)), _ray((0, 0, 0), (np.inf, 0, 1)),
                     _ray((0, 0, 0), (0, 0, 1), 2.0, 1.0), _ray((0, 0, 0), (0, 0, 1), 0.0, np.nan),
                     _ray((1e30, 0, 0), (1, 0, 0)), _ray((0.5, 0.5, -3e38), (0, 0, 3e38))], f32)


def flatten(arrays, translations):
    """The scene copied once per translation, copies in order (flat triangle id = copy * T + id): (positions, ..., meshes)"""
    P, N, T, I, M = arrays
    Ps, Ns, Ts, Is, Ms = [], [], [], [], []
    for k, t in enumerate(np.asarray(translations, f32)):
        for m in np.asarray(M, np.uint32).reshape(-1, 8):
            nv, fv, ni, fi = (int(x) for x in m[:4])
            Ms.append([nv, fv + k * len(P), ni, fi + k * len(I), len(Ms), m[5], 0, 0])
        Ps.append(np.asarray(P, f32) + t), Ns.append(N), Ts.append(T), Is.append(I)
    return (np.concatenate(Ps).astype(f32), np.concatenate(Ns), np.concatenate(Ts), np.concatenate(Is), np.array(Ms, np.uint32))


def grid_scene(n=30, seed=11):
    """n*2 triangles with vertices on multiples of 1/16, |value| < 8, overlapping at random (for the exact flattening identity)"""
    rng = np.random.default_rng(seed)
    P = (rng.integers(-64, 65, (4 * n, 3)) / 16.0).astype(f32)
    I = np.concatenate([[4 * q, 4 * q + 1, 4 * q + 2, 4 * q, 4 * q + 2, 4 * q + 3] for q in range(n)]).astype(np.uint32)
    N, T = np.tile(f32([0, 0, 1]), (len(P), 1)), np.zeros((len(P), 2), f32)
    M = np.array([[len(P), 0, len(I), 0, 0, 0xFFFFFFFF, 0, 0]], np.uint32)
    return (P, N, T, I, M), P[I.astype(np.int64)].reshape(-1, 3, 3)


def grid_rays(n, centres, seed=12):
    """origins on multiples of 1/16 with |value| < 128, arbitrary directions towards the neighbourhood of one of the centres"""
    rng = np.random.default_rng(seed)
    o = rng.integers(-127 * 16, 127 * 16 + 1, (n, 3)) / 16.0
    aim = np.asarray(centres, np.float64)[rng.integers(len(centres), size=n)] + rng.uniform(-4, 4, (n, 3))
    return np.c_[o, np.zeros(n), aim - o, np.full(n, np.inf)].astype(f32)


def translations(T):
    """(n, 3, 4) float32 pure translations"""
    T = np.asarray(T, f32)
    M = np.tile(np.c_[np.eye(3), np.zeros(3)].astype(f32), (len(T), 1, 1))
    M[:, :, 3] = T
    return M
