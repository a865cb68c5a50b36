"""Helpers of the closest-point query tests (cap_closest_points): the per-triangle function of include/capsaicin_hip.h transcribed to
numpy, vectorised over points x triangles -- one rounded operation per line of the contract, float32 throughout on the answer path (the
same code runs in float64 as the twin the reference is judged against) -- the (dist2, id) argmin under a radius and a per-triangle
mask, the expected 32-byte records, and scene makers."""
import numpy as np

from capsaicin_amd import capi

MISS = capi.MISS
EPS = np.float64(2.0 ** -24)  # unit roundoff of binary32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def records_of(tris, dtype=np.float32):
    """(v0, e1, e2) as the device stores them: e1 = v1 - v0, e2 = v2 - v0, one rounded subtraction each, from (T, 3, 3) vertices"""
    t = np.asarray(tris, dtype)
    return t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cascade(p, v0, e1, e2):
    """The contract for points p (N, 3) against records (T, 3) each, in the arrays' own dtype: dist2, u, v (N, T), feature (N, T) uint32
    and the closest points (N, T, 3).  Every symbol is evaluated for every pair (they are pure functions of the pair); the cases are
    applied last to first, so the first matching one wins."""
    dt = p.dtype
    assert v0.dtype == dt and e1.dtype == dt and e2.dtype == dt
    one, zero = dt.type(1), dt.type(0)
    with np.errstate(all="ignore"):
        ap = p[:, None, :] - v0[None]
        E1, E2 = e1[None], e2[None]
        d1, d2 = _dot(E1, ap), _dot(E2, ap)
        bp = ap - E1
        d3, d4 = _dot(E1, bp), _dot(E2, bp)
        vc = d1 * d4 - d3 * d2
        cp = ap - E2
        d5, d6 = _dot(E1, cp), _dot(E2, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        a43, a56 = d4 - d3, d5 - d6
        s = (va + vb) + vc
        u, v = vb / s, vc / s
        f = np.zeros(u.shape, np.uint32)

        def case(cond, cu, cv, feature):
            nonlocal u, v, f
            u, v, f = np.where(cond, cu, u).astype(dt), np.where(cond, cv, v).astype(dt), np.where(cond, np.uint32(feature), f)

        w = a43 / (a43 + a56)
        case((va <= 0) & (a43 >= 0) & (a56 >= 0), one - w, w, 2)
        case((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6), 3)
        case((d6 >= 0) & (d5 <= d6), zero, one, 6)
        case((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero, 1)
        case((d3 >= 0) & (d4 <= d3), one, zero, 5)
        case((d1 <= 0) & (d2 <= 0), zero, zero, 4)
        m = E1 * u[..., None] + E2 * v[..., None]
        delta = ap - m
        dist2 = _dot(delta, delta)
        point = v0[None] + m
    assert dist2.dtype == dt and u.dtype == dt and point.dtype == dt
    return dist2, u, v, f, point


def degenerate(points):
    """queries that are not traversed: a non-finite coordinate, a radius that is NaN or negative"""
    q = np.asarray(points, np.float32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(q[:, 0:3]).all(1) & (q[:, 3] >= 0))


def argmin_lex(dist2, valid):
    """per row the lowest index among the valid entries of minimal dist2, -1 without a valid entry"""
    with np.errstate(invalid="ignore"):
        key = np.where(valid, dist2, np.inf)
    idx = np.argmin(key, axis=1)  # (the first occurrence: the lowest id)
    rows = np.arange(len(idx))
    some = valid.any(1)
    stray = some & ~valid[rows, idx]  # every valid dist2 is +inf and an invalid entry came first
    idx[stray] = np.argmax(valid[stray], axis=1)
    return np.where(some, idx, -1)


def closest(points, tris, mask=None, chunk=128, ids=None):
    """The expected (N, 8) float32 records of cap_closest_points for (N, 4) queries over (T, 3, 3) float32 triangles in global id order.
    mask: per-triangle bool, False = filtered out.  Also returns the (N, T) float32 dist2 table (NaN where masked out)."""
    q = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    tris = np.ascontiguousarray(tris, np.float32)
    v0, e1, e2 = records_of(tris)
    out = np.zeros((len(q), 8), np.float32)
    ob = out.view(np.uint32)
    table = np.zeros((len(q), len(tris)), np.float32)
    r2 = q[:, 3] * q[:, 3]
    assert r2.dtype == np.float32
    bad = degenerate(q)
    for s in range(0, len(q), chunk):
        e = min(len(q), s + chunk)
        d2, u, v, f, pt = cascade(q[s:e, 0:3], v0, e1, e2)
        if mask is not None:
            d2 = np.where(np.asarray(mask, bool)[None], d2, np.float32(np.nan))
        table[s:e] = d2
        with np.errstate(invalid="ignore"):
            valid = d2 <= r2[s:e, None]
        valid &= ~bad[s:e, None]
        g = argmin_lex(d2, valid)
        for k in range(e - s):
            i = s + k
            if g[k] < 0:
                out[i, 3] = 0.0 if bad[i] else r2[i]
                ob[i, 6] = MISS
                continue
            out[i, 0:3], out[i, 3], out[i, 4], out[i, 5] = pt[k, g[k]], d2[k, g[k]], u[k, g[k]], v[k, g[k]]
            ob[i, 6], ob[i, 7] = g[k], f[k, g[k]]
    return out, table


def assert_records(got, want, what=""):
    """bit for bit on all eight words"""
    g, w = bits(got).reshape(-1, 8), bits(want).reshape(-1, 8)
    bad = np.nonzero((g != w).any(1))[0]
    assert len(bad) == 0, "%s: %d of %d records differ, first %d: got %s (%s) want %s (%s)" % (
        what, len(bad), len(g), bad[0], got.reshape(-1, 8)[bad[0]].tolist(), g[bad[0], 6:8].tolist(), want.reshape(-1, 8)[bad[0]].tolist(), w[bad[0], 6:8].tolist())


def queries(xyz, radius=np.inf):
    q = np.zeros((len(xyz), 4), np.float32)
    q[:, 0:3], q[:, 3] = xyz, radius
    return q


# ---- scenes ----
def arrays(*tri_sets):
    """GeometryStorage arrays (positions, normals, texcoords, indices, meshes) of one mesh per (T, 3, 3) triangle set, three vertices per
    triangle in order: global triangle ids run through the sets in the order given"""
    P, I, D = [], [], []
    fv = fi = 0
    for t in tri_sets:
        t = np.ascontiguousarray(t, np.float32).reshape(-1, 3, 3)
        P.append(t.reshape(-1, 3))
        I.append(np.arange(3 * len(t), dtype=np.uint32))
        D.append([3 * len(t), fv, 3 * len(t), fi, len(D), 0xFFFFFFFF, 0, 0])  # (field 4: the mesh's own slot)
        fv += 3 * len(t)
        fi += 3 * len(t)
    P = np.concatenate(P)
    N = np.tile(np.float32([0, 0, 1]), (len(P), 1))
    return P, N, np.zeros((len(P), 2), np.float32), np.concatenate(I), np.array(D, np.uint32)


def context(tri_sets, build=None):
    r = capi.Renderer(0)
    if build is not None:
        r.set_bvh_build(build)
    r.upload_scene(*arrays(*tri_sets))
    r.build_bvh()
    return r


def soup(rng, n, edge=0.05, lo=0.0, hi=1.0, offset=0.0, min_shape=0.2):
    """n triangles with centres uniform in [lo, hi]^3 + offset and edges around `edge`, none thinner than min_shape (shortest altitude
    over longest edge, before rounding to float32)"""
    out = np.zeros((0, 3, 3))
    while len(out) < n:
        c = lo + rng.random((2 * n, 1, 3)) * (hi - lo)
        t = c + (rng.random((2 * n, 3, 3)) - 0.5) * edge
        e = np.stack([t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 0] - t[:, 2]], 1)
        longest = np.linalg.norm(e, axis=2).max(1)
        area2 = np.linalg.norm(np.cross(e[:, 0], -e[:, 2]), axis=1)
        out = np.concatenate([out, t[area2 / longest / longest >= min_shape]])
    return (out[:n] + offset).astype(np.float32)


def sphere(rows=50, cols=50, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """a latitude / longitude sphere of 2 * cols * (rows - 1) triangles (4 900 by default)"""
    th = np.linspace(0.0, np.pi, rows + 1)
    ph = np.linspace(0.0, 2.0 * np.pi, cols + 1)
    def at(i, j):
        return np.array([np.sin(th[i]) * np.cos(ph[j % cols]), np.sin(th[i]) * np.sin(ph[j % cols]), np.cos(th[i])]) * radius + np.array(centre)
    out = []
    for i in range(rows):
        for j in range(cols):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            if i > 0:
                out.append((a, b, d))
            if i < rows - 1:
                out.append((b, c, d))
    return np.array(out).astype(np.float32)


def needles(rng, n, length=0.2, aspect=1e4):
    """n triangles of the given aspect ratio (long edge over height), random directions, centres in the unit cube"""
    c = rng.random((n, 1, 3))
    a = rng.normal(size=(n, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(a, rng.normal(size=(n, 3)))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    s = rng.random((n, 1))  # where along the long edge the apex stands
    t = np.stack([-0.5 * length * a, 0.5 * length * a, (s - 0.5) * length * a + (length / aspect) * b], 1)
    return (c + t).astype(np.float32)


def around(rng, tris, n, spread=0.5):
    """n points uniform in the triangles' box grown by `spread` of its extent on every side: inside and outside"""
    lo, hi = tris.reshape(-1, 3).min(0).astype(np.float64), tris.reshape(-1, 3).max(0).astype(np.float64)
    ext = np.maximum(hi - lo, 1e-3)
    return (lo - spread * ext + rng.random((n, 3)) * (1 + 2 * spread) * ext).astype(np.float32)


def near_surface(rng, tris, n, off=1e-3):
    """n points displaced by up to `off` from random points of random triangles"""
    g = rng.integers(0, len(tris), n)
    b = rng.dirichlet((1, 1, 1), n)
    p = np.einsum("nk,nkj->nj", b, tris[g].astype(np.float64))
    return (p + (rng.random((n, 3)) - 0.5) * 2 * off).astype(np.float32)
