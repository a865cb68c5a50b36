"""Helpers of the multi-hit query tests (cap_trace_rays_multi): a stack of parallel quads, every hit of a ray by the oracle's triangle
test in the contract's (t, triangle) order, the pages and counts that follow from it, and float64 candidate supersets for large
scenes."""
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


def stacked_quads(n=40, dz=0.25):
    """n unit quads in the planes z = i * dz, each two triangles sharing the diagonal (0, 0) - (1, 1): triangle 2i = (0,0) (1,0) (1,1)
    covers y <= x, 2i + 1 = (0,0) (1,1) (0,1) covers y >= x.  Returns (positions, normals, texcoords, indices, meshes) and the
    (2n, 3, 3) triangles in global id order."""
    P, I = [], []
    for i in range(n):
        z = i * dz
        b = len(P)
        P += [(0, 0, z), (1, 0, z), (1, 1, z), (0, 1, z)]
        I += [b, b + 1, b + 2, b, b + 2, b + 3]
    P = np.array(P, np.float32)
    I = np.array(I, np.uint32)
    N = np.tile(np.float32([0, 0, 1]), (len(P), 1))
    T = np.zeros((len(P), 2), np.float32)
    meshes = np.array([[len(P), 0, len(I), 0, 0, 0xFFFFFFFF, 0, 0]], np.uint32)
    return (P, N, T, I, meshes), P[I.astype(np.int64)].reshape(-1, 3, 3)


def all_hits(ray, tris, cands=None):
    """Every hit of the intersection contract among the candidates (all triangles by default) as (t, u, v, id), float32 values from
    the oracle's test, sorted by (t, id)."""
    from oracle import cap_oracle as O
    o, d, tmin, tmax = ray[0:3], ray[4:7], float(ray[3]), float(ray[7])
    out = []
    for g in (range(len(tris)) if cands is None else sorted(set(int(c) for c in cands))):
        h = O.intersect_triangle(o, d, tmin, tmax, tris[g, 0], tris[g, 1], tris[g, 2])
        if h is not None:
            out.append((np.float32(h[0]), np.float32(h[1]), np.float32(h[2]), g))
    out.sort(key=lambda x: (x[0], x[3]))
    return out


def records(hits, k, tmax):
    """(k, 4) float32 page of the first k hits, miss records (tmax, 0, 0, MISS) after the last"""
    page = np.zeros((k, 4), np.float32)
    page[:, 0] = tmax
    page.view(np.uint32)[:, 3] = MISS
    for j, (t, u, v, g) in enumerate(hits[:k]):
        page[j, 0:3] = (t, u, v)
        page.view(np.uint32)[j, 3] = g
    return page


def after(hits, cursor):
    """the hits after the cursor record (t_c, ., ., g_c) in (t, id) order"""
    tc, gc = np.float32(cursor[0]), int(bits(cursor)[3])
    return [h for h in hits if h[0] > tc or (h[0] == tc and h[3] > gc)]


def expected_pages(rays, lists, k):
    """(N, k, 4) pages and (N,) counts from per-ray hit lists"""
    return (np.stack([records(h, k, r[7]) for r, h in zip(rays, lists)]) if k else np.zeros((len(rays), 0, 4), np.float32),
            np.array([len(h) for h in lists], np.int32))


def page_to_exhaustion(r, rays, k, limit=200):
    """Pages of k records until every ray's page is empty; returns the per-ray concatenation (records before the first miss) and the
    pages themselves."""
    page = r.trace_rays_multi(rays, k)
    pages = [page.copy()]
    for _ in range(limit):
        if np.all(bits(page)[:, 0, 3] == MISS):
            break
        page = r.trace_rays_multi(rays, k, resume=page)
        pages.append(page.copy())
    else:
        raise AssertionError("paging did not end")
    walked = []
    for i in range(len(rays)):
        recs = np.concatenate([p[i] for p in pages])
        walked.append(recs[bits(recs)[:, 3] != MISS])
    return walked, pages


def hit_list_array(hits):
    return records(hits, len(hits), 0.0) if hits else np.zeros((0, 4), np.float32)


def candidate_superset(rays, tris, margin=1e-4, chunk=8192, nearest=False):
    """Per ray, every triangle whose float64 intersection (with a relative margin on the barycentrics and on both ends of the
    interval) lies in the ray's interval: a superset of the triangles the float32 contract can accept (torch float64 on the GPU).
    nearest=True keeps only those within the margin of the nearest such t, the candidates of a closest-hit record -- the form of
    refit_support.candidates and test_ray_query_gpu.candidates, which this generalises."""
    import torch
    dev = torch.device("cuda", 0)
    R = torch.as_tensor(np.ascontiguousarray(rays, np.float32), device=dev).double()
    o, tmin, d, tmax = R[:, 0:3], R[:, 3], R[:, 4:7], R[:, 7]
    T = torch.as_tensor(tris, device=dev).double()
    best = torch.full((len(rays),), float("inf"), dtype=torch.float64, device=dev)
    ts = []
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
        ts.append(t)
    out = [[] for _ in range(len(rays))]
    for k, t in enumerate(ts):
        keep = torch.isfinite(t)
        if nearest:
            keep &= t <= (best + margin * (1.0 + best.abs()))[:, None]
        ri, ti = torch.nonzero(keep, as_tuple=True)
        for a, b in zip(ri.tolist(), (ti + k * chunk).tolist()):
            out[a].append(b)
    return out
