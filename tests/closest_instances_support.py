"""Helpers of the instanced closest-point tests (cap_closest_instances): the world record of include/capsaicin_hip.h in single-rounded
float32 operations (the same code in float64 is the twin), closest_point_support.cascade over every (instance, triangle), the argmin in
(dist2, instance, triangle) order under the masks, the object ranges and the radius, and the debug entry's wrapper."""
import ctypes as C

import numpy as np

from closest_point_support import MISS, argmin_lex, assert_records, bits, cascade, degenerate, records_of  # noqa: F401
from instance_support import regular_transforms, rotation  # noqa: F401

EPS = np.float64(2.0 ** -24)


def _dot_c(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z for rows a (I, 1, 3) against records b (1, T, 3)"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def world_records(M, tris, dtype=np.float32):
    """(v0w, e1w, e2w), each (I, T, 3), of the (T, 3, 3) triangles under the (I, 3, 4) transforms, by the contract's rule"""
    M = np.asarray(M, np.float32).reshape(-1, 3, 4).astype(dtype)
    v0, e1, e2 = (x[None] for x in records_of(np.asarray(tris, np.float32), dtype))
    with np.errstate(all="ignore"):
        v0w = np.stack([_dot_c(M[:, None, r, :3], v0) + M[:, None, r, 3] for r in range(3)], -1)
        e1w = np.stack([_dot_c(M[:, None, r, :3], e1) for r in range(3)], -1)
        e2w = np.stack([_dot_c(M[:, None, r, :3], e2) for r in range(3)], -1)
    assert v0w.dtype == dtype and e1w.dtype == dtype
    return v0w, e1w, e2w


def live_of(M):
    """what cap_instances_set would keep: finite, invertible, kappa within the limit -- through the debug entry (W = 0 when inert)"""
    return np.array([bound(m, (0, 0, 0), (0, 0, 0), (0, 0, 0), 0.0)["g"] > 0 for m in np.asarray(M, np.float32).reshape(-1, 3, 4)])


def pair_valid(n_inst, n_tris, live=None, inst_masks=None, tri_mesh_masks=None, mask=None, obj_of_inst=None, obj_of_tri=None):
    """(I, T) bool: the pairs that may be candidates at all"""
    ok = np.ones((n_inst, n_tris), bool)
    if live is not None:
        ok &= np.asarray(live, bool)[:, None]
    im = np.full(n_inst, 0xFF, np.uint32) if inst_masks is None else np.asarray(inst_masks, np.uint32)
    tm = np.full(n_tris, 0xFF, np.uint32) if tri_mesh_masks is None else np.asarray(tri_mesh_masks, np.uint32)
    call = 0xFF if not mask else int(mask)
    ok &= (im[:, None] & tm[None, :] & np.uint32(call)) != 0
    if obj_of_inst is not None:
        ok &= np.asarray(obj_of_inst)[:, None] == np.asarray(obj_of_tri)[None, :]
    return ok


def closest_instances(points, M, tris, valid=None, chunk=64, dtype=np.float32, with_table=False):
    """(records (N, 8) float32, instances (N,) int32 with -1 on a miss[, dist2 table (N, I, T)]) of the brute force.  valid: (I, T)
    bool from pair_valid, None = every pair.  dtype=float64 is the twin: the same rule in double (its records are rounded to float32
    only when stored; the table keeps the doubles)."""
    q = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    M = np.asarray(M, np.float32).reshape(-1, 3, 4)
    tris = np.ascontiguousarray(tris, np.float32)
    I, T = len(M), len(tris)
    if valid is None:
        valid = np.ones((I, T), bool)
    v0w, e1w, e2w = (x.reshape(I * T, 3) for x in world_records(M, tris, dtype))
    out = np.zeros((len(q), 8), np.float32)
    ob = out.view(np.uint32)
    inst = np.full(len(q), -1, np.int32)
    table = np.zeros((len(q), I, T), dtype) if with_table else None
    r2 = (q[:, 3] * q[:, 3]).astype(dtype)
    bad = degenerate(q)
    flat_valid = valid.reshape(-1)
    for s in range(0, len(q), chunk):
        e = min(len(q), s + chunk)
        d2, u, v, f, pt = cascade(q[s:e, 0:3].astype(dtype), v0w, e1w, e2w)
        if with_table:
            table[s:e] = d2.reshape(e - s, I, T)
        with np.errstate(invalid="ignore"):
            ok = (d2 <= r2[s:e, None]) & flat_valid[None] & ~bad[s:e, None]
        k = argmin_lex(d2, ok)  # (the flat index i * T + g orders ties by (i, g))
        for a in range(e - s):
            i = s + a
            if k[a] < 0:
                out[i, 3] = 0.0 if bad[i] else q[i, 3] * q[i, 3]
                ob[i, 6] = MISS
                continue
            out[i, 0:3], out[i, 3], out[i, 4], out[i, 5] = pt[a, k[a]], d2[a, k[a]], u[a, k[a]], v[a, k[a]]
            ob[i, 6], ob[i, 7] = k[a] % T, f[a, k[a]]
            inst[i] = k[a] // T
    return (out, inst, table) if with_table else (out, inst)


def assert_pairs(got, want, what=""):
    """records bit for bit on all eight words, and the instance"""
    (g_rec, g_inst), (w_rec, w_inst) = got, want
    assert_records(g_rec, w_rec, what)
    bad = np.nonzero(np.asarray(g_inst, np.int64) != np.asarray(w_inst, np.int64))[0]
    assert len(bad) == 0, "%s: %d instances differ, first %d: got %d want %d" % (what, len(bad), bad[0], g_inst[bad[0]], w_inst[bad[0]])


def flat_record(rec, inst, T):
    """the instanced records renumbered as the flattened scene's: flat id = i * T + g"""
    out = np.array(rec, np.float32, copy=True)
    ob = out.view(np.uint32)
    hit = np.asarray(inst) >= 0
    ob[hit, 6] = (np.asarray(inst)[hit].astype(np.int64) * T + ob[hit, 6]).astype(np.uint32)
    return out


def triangles_of(arrays):
    """(T, 3, 3) float32 triangles of GeometryStorage arrays (positions, normals, texcoords, indices, meshes) in global id order"""
    P, _, _, I, M = arrays
    P, I = np.asarray(P, np.float32).reshape(-1, 3), np.asarray(I).astype(np.int64)
    return np.concatenate([P[I[int(d[3]):int(d[3]) + int(d[2])] + int(d[1])].reshape(-1, 3, 3) for d in np.asarray(M).reshape(-1, 8)])


# ---- the debug entry ----
def bound(M, box_lo, box_hi, point, best, lib=None):
    """cap_debug_closest_instance_bound for one transform, box, point and best dist2: {W, g, xw, slack, skip}"""
    if lib is None:
        from capsaicin_amd import capi
        lib = capi.lib()
    f3 = C.c_float * 3
    m = (C.c_float * 12)(*np.asarray(M, np.float32).reshape(12).tolist())
    W = (C.c_float * 12)()
    g, xw, slack, skip = C.c_float(), C.c_float(), C.c_float(), C.c_uint32()
    rc = lib.cap_debug_closest_instance_bound(m, f3(*np.float32(box_lo).tolist()), f3(*np.float32(box_hi).tolist()), f3(*np.float32(point).tolist()),
                                              C.c_float(float(np.float32(best))), W, C.byref(g), C.byref(xw), C.byref(slack), C.byref(skip))
    assert rc == 0, lib.cap_last_error()
    return dict(W=np.array(W[:], np.float32).reshape(3, 4), g=g.value, xw=xw.value, slack=slack.value, skip=int(skip.value))


# ---- transforms ----
def affine(L, t=(0, 0, 0)):
    return np.c_[np.asarray(L, np.float64), np.asarray(t, np.float64)].astype(np.float32)


def identity(n=1):
    return np.tile(affine(np.eye(3)), (n, 1, 1))


def near_translations(M, offset=4096.0):
    """the transforms with their translations moved to the neighbourhood of `offset`"""
    out = np.array(M, np.float32, copy=True)
    out[:, :, 3] = (out[:, :, 3] * np.float32(0.05) + np.float32(offset)).astype(np.float32)
    return out


def world_points_near(rng, M, tris, n, off=1e-3):
    """n world points within `off` (relative to the instance's scale) of random points of random triangles of random instances"""
    M = np.asarray(M, np.float64)
    i = rng.integers(0, len(M), n)
    g = rng.integers(0, len(tris), n)
    b = rng.dirichlet((1, 1, 1), n)
    x = np.einsum("nk,nkj->nj", b, np.asarray(tris, np.float64)[g])
    y = np.einsum("nrk,nk->nr", M[i][:, :, :3], x) + M[i][:, :, 3]
    scale = np.linalg.norm(M[i][:, :, :3], axis=(1, 2))
    return (y + (rng.random((n, 3)) - 0.5) * 2 * off * scale[:, None]).astype(np.float32)


def world_hull_points(rng, M, tris, n, grow=0.1):
    """n points uniform in the box of every instance's image of the triangles' box, grown by `grow` of its extent"""
    lo, hi = tris.reshape(-1, 3).min(0).astype(np.float64), tris.reshape(-1, 3).max(0).astype(np.float64)
    corners = np.array([[(hi if (c >> k) & 1 else lo)[k] for k in range(3)] for c in range(8)])
    w = np.einsum("irk,ck->icr", np.asarray(M, np.float64)[:, :, :3], corners) + np.asarray(M, np.float64)[:, None, :, 3]
    wlo, whi = w.reshape(-1, 3).min(0), w.reshape(-1, 3).max(0)
    ext = whi - wlo
    return (wlo - grow * ext + rng.random((n, 3)) * (1 + 2 * grow) * ext).astype(np.float32)


def instance_box_points(rng, M, tris, n, grow=0.5):
    """n points, point k uniform in the box of instance (k mod I)'s image of the triangles' box grown by `grow` of its extent"""
    lo, hi = tris.reshape(-1, 3).min(0).astype(np.float64), tris.reshape(-1, 3).max(0).astype(np.float64)
    corners = np.array([[(hi if (c >> k) & 1 else lo)[k] for k in range(3)] for c in range(8)])
    Md = np.asarray(M, np.float64)
    w = np.einsum("irk,ck->icr", Md[:, :, :3], corners) + Md[:, None, :, 3]
    i = np.arange(n) % len(Md)
    wlo, whi = w.min(1)[i], w.max(1)[i]
    ext = whi - wlo
    return (wlo - grow * ext + rng.random((n, 3)) * (1 + 2 * grow) * ext).astype(np.float32)
