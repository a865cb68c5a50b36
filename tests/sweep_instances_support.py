"""Helpers of the instanced sphere sweep tests (cap_sweep_instances): the brute force -- closest_instances_support.world_records composed
with sweep_support.sweep_pairs over every (instance, triangle), the argmin in (t, instance, triangle) order under pair_valid --, its
float64 twin, the aimed sweeps of the soup tests, the debug entry's wrapper and a numpy model of the walk's world-space prune."""
import ctypes as C

import numpy as np

from closest_instances_support import (affine, assert_pairs, flat_record, identity, live_of, near_translations, pair_valid,  # noqa: F401
                                       world_records)
from closest_point_support import MISS, argmin_lex, bits  # noqa: F401
from sweep_support import SLACK, degenerate, slab_times, sweep_pairs, sweep_queries

f32 = np.float32
EPS32 = f32(2.0 ** -24)


def sweep_instances(sweeps, M, tris, valid=None, chunk=128, dtype=np.float32):
    """(records (N, 8) float32, instances (N,) int32 with -1 on a miss, time table (N, I, T) with +inf where a pair has no contact or
    is not valid) of the brute force.  valid: (I, T) bool from pair_valid, None = every pair.  dtype=float64 is the twin: the same
    rule in double on the same binary32 inputs (its records are rounded to float32 only when stored; the table keeps the doubles)."""
    q = np.ascontiguousarray(sweeps, f32).reshape(-1, 8)
    M = np.asarray(M, f32).reshape(-1, 3, 4)
    tris = np.ascontiguousarray(tris, f32)
    I, T = len(M), len(tris)
    flat_valid = np.ones(I * T, bool) if valid is None else np.asarray(valid, bool).reshape(-1)
    v0w, e1w, e2w = (np.ascontiguousarray(x.reshape(I * T, 3)) for x in world_records(M, tris, dtype))
    out = np.zeros((len(q), 8), f32)
    ob = out.view(np.uint32)
    inst = np.full(len(q), -1, np.int32)
    table = np.full((len(q), I, T), np.inf, dtype)
    bad = degenerate(q)
    for s in range(0, len(q), chunk):
        e = min(len(q), s + chunk)
        contact, t, pt, u, v, f, _ = sweep_pairs(q[s:e].astype(dtype), v0w, e1w, e2w)
        contact = contact & flat_valid[None] & ~bad[s:e, None]
        table[s:e] = np.where(contact, t, dtype(np.inf)).reshape(e - s, I, T)
        k = argmin_lex(t, contact)  # (the flat index i * T + g orders ties by (i, g))
        for a in range(e - s):
            i = s + a
            if k[a] < 0:
                out[i, 3] = 0.0 if bad[i] else q[i, 7]
                ob[i, 6] = MISS
                continue
            out[i, 0:3], out[i, 3], out[i, 4], out[i, 5] = pt[a, k[a]], t[a, k[a]], u[a, k[a]], v[a, k[a]]
            ob[i, 6], ob[i, 7] = k[a] % T, f[a, k[a]]
            inst[i] = k[a] // T
    return out, inst, table


def expected(sweeps, M, tris, valid=None):
    """(records, instances) alone: what assert_pairs takes"""
    return sweep_instances(sweeps, M, tris, valid)[:2]


# ---- the world boxes of the instances, in float64 ----
def instance_world_boxes(M, tris):
    """(lo, hi), each (I, 3): the box of every instance's image of the triangles' box"""
    lo, hi = tris.reshape(-1, 3).min(0).astype(np.float64), tris.reshape(-1, 3).max(0).astype(np.float64)
    corners = np.array([[(hi if (c >> k) & 1 else lo)[k] for k in range(3)] for c in range(8)])
    Md = np.asarray(M, np.float64).reshape(-1, 3, 4)
    w = np.einsum("irk,ck->icr", Md[:, :, :3], corners) + Md[:, None, :, 3]
    return w.min(1), w.max(1)


def aimed_sweeps(rng, M, tris, n, radius, grow=0.5, jitter=0.05, origin_scale=1.0):
    """n sweeps, sweep k from a point of the world box of instance k mod I grown by `grow` of its extent, aimed near a point of a
    triangle of that instance (within `jitter` of the instance's size), the direction scaled by 0.5 .. 2; radius in units of the
    instance's size; a third each with tmax = inf, a tmax about the instance's size and a short one.  origin_scale > 1 moves the origin
    away from the target along the line by that many instance sizes (for origins far away)."""
    Md = np.asarray(M, np.float64).reshape(-1, 3, 4)
    T = np.asarray(tris, np.float64)
    wlo, whi = instance_world_boxes(Md, tris)
    i = np.arange(n) % len(Md)
    ext = (whi - wlo)[i]
    size = ext.max(1)
    o = wlo[i] - grow * ext + rng.random((n, 3)) * (1 + 2 * grow) * ext
    g = rng.integers(0, len(T), n)
    b = rng.dirichlet((1, 1, 1), n)
    x = np.einsum("nk,nkj->nj", b, T[g])
    y = np.einsum("nrk,nk->nr", Md[i][:, :, :3], x) + Md[i][:, :, 3] + rng.normal(size=(n, 3)) * jitter * size[:, None]
    d = y - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
    if origin_scale != 1.0:
        o = y - d * origin_scale * size[:, None]
    d *= 0.5 + 1.5 * rng.random((n, 1))
    third = np.arange(n) // len(Md) % 3
    tmax = np.where(third == 0, np.inf, np.where(third == 1, size, 0.2 * size))
    return sweep_queries(o, radius * size, d, tmax)


# ---- the debug entry ----
def _f(values, n):
    return (C.c_float * n)(*np.asarray(values, f32).reshape(n).tolist())


def sweep_prune(M, object_lo, object_hi, node_lo, node_hi, sweep, far, lib=None):
    """cap_debug_sweep_instance_prune for one transform, object box, object-space node box, sweep and far bound:
    {xw, radius, world_lo, world_hi, entry, exit, skip}"""
    if lib is None:
        from capsaicin_amd import capi
        lib = capi.lib()
    wlo, whi = (C.c_float * 3)(), (C.c_float * 3)()
    xw, radius, entry, ex, skip = C.c_float(), C.c_float(), C.c_float(), C.c_float(), C.c_uint32()
    rc = lib.cap_debug_sweep_instance_prune(_f(M, 12), _f(object_lo, 3), _f(object_hi, 3), _f(node_lo, 3), _f(node_hi, 3), _f(sweep, 8),
                                            C.c_float(float(f32(far))), C.byref(xw), C.byref(radius), wlo, whi, C.byref(entry), C.byref(ex),
                                            C.byref(skip))
    assert rc == 0, lib.cap_last_error()
    return dict(xw=f32(xw.value), radius=f32(radius.value), world_lo=np.array(wlo[:], f32), world_hi=np.array(whi[:], f32), entry=f32(entry.value),
                exit=f32(ex.value), skip=int(skip.value))


# ---- the prune, as sweep.hip and cap_near.h have it (float32 throughout) ----
def world_extent(M, object_lo, object_hi):
    """Xw of cap_near.h near_world_extent: per row the sum of the magnitudes of the terms, in double, rounded upwards"""
    m = np.asarray(M, f32).reshape(3, 4).astype(np.float64)
    xmax = np.maximum(np.abs(np.asarray(object_lo, f32).astype(np.float64)), np.abs(np.asarray(object_hi, f32).astype(np.float64)))
    x = 0.0
    for r in range(3):
        row = abs(m[r, 3])
        for k in range(3):
            row += abs(m[r, k]) * xmax[k]
        x = max(x, row)
    return np.nextafter(f32(x), f32(np.inf))


def prune_radius(sweep, xw):
    """R = fl(r + fl(128 eps . fl(fl(|o|_inf + Xw) + r)))"""
    q = np.asarray(sweep, f32)
    with np.errstate(all="ignore"):
        return q[3] + (f32(SLACK) * EPS32) * ((np.max(np.abs(q[0:3])) + f32(xw)) + q[3])


def world_box(M, lo, hi):
    """overlap_world_box of cap_near.h: the world box of the object-space box [lo, hi] under M, centre and half-extent form"""
    m = np.asarray(M, f32).reshape(3, 4)
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    with np.errstate(all="ignore"):
        hl, hh = lo * f32(0.5), hi * f32(0.5)
        c, h = hl + hh, hh - hl
        cw = ((m[:, 0] * c[0] + m[:, 1] * c[1]) + m[:, 2] * c[2]) + m[:, 3]
        hw = (np.abs(m[:, 0]) * h[0] + np.abs(m[:, 1]) * h[1]) + np.abs(m[:, 2]) * h[2]
        return cw - hw, cw + hw


def prune_model(M, object_lo, object_hi, node_lo, node_hi, sweep, far):
    """the numpy model of the debug entry for a live transform: the same dict"""
    q = np.asarray(sweep, f32)
    xw = world_extent(M, object_lo, object_hi)
    R = prune_radius(q, xw)
    wlo, whi = world_box(M, node_lo, node_hi)
    with np.errstate(all="ignore"):
        inv = f32(1.0) / q[4:7]
    tn, ex = slab_times(q[0:3], inv, R, wlo, whi, f32(far))
    return dict(xw=xw, radius=R, world_lo=wlo, world_hi=whi, entry=f32(tn), exit=f32(ex), skip=0 if tn <= ex else 1)
