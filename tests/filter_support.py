"""Helpers of the ray-flag / instance-mask query tests (cap_trace_*_ex): the facing of a triangle for a ray in the contract's own fp32
arithmetic, the brute-force filtered hit set every GPU record is compared with, and a stack of quads with one mesh per quad."""
import ctypes

import numpy as np

from multi_hit_support import MISS, all_hits, bits, records  # noqa: F401  (re-exported for the tests)

_fmaf = ctypes.CDLL("libm.so.6").fmaf
_fmaf.restype, _fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
f32 = np.float32


def fma(a, b, c):
    """fmaf(a, b, c): one rounding"""
    return f32(_fmaf(float(a), float(b), float(c)))


def _dot(a, b):  # oracle/cap_oracle.cpp dot(): fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))
    return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0]))


def _cross(a, b):  # oracle/cap_oracle.cpp cross(): fmaf(a.y, b.z, -(a.z * b.y)), ...
    return (fma(a[1], b[2], -(a[2] * b[1])), fma(a[2], b[0], -(a[0] * b[2])), fma(a[0], b[1], -(a[1] * b[0])))


def facing(ray, tri):
    """+1 front-facing (det > 0), -1 back-facing (det < 0), 0 (det == 0, no hit) with the contract's det = -dot(d, n), n = e1 x e2,
    e = v - v0, every operation a single-rounded float32 one (np.float32 for + - x, libm's fmaf where the contract writes fmaf):
    the arithmetic of the oracle's triangle set-up and test, so the sign is exactly the one the kernels' tri_test sees."""
    with np.errstate(all="ignore"):
        v0, v1, v2 = (np.asarray(tri[k], f32) for k in range(3))
        e1, e2 = v1 - v0, v2 - v0
        d = np.asarray(ray[4:7], f32)
        det = -_dot(d, _cross(e1, e2))
    return 1 if det > 0 else (-1 if det < 0 else 0)


def occludes(ray, tri):
    """The occlusion form of the contract's test (the oracle's occludes_tri, the kernels' tri_occludes) in the same exact fp32
    arithmetic as facing(): det > 0 after the two-sided flip, U, V >= 0, U + V <= det, tmin * det < T < tmax * det."""
    with np.errstate(all="ignore"):
        v0, v1, v2 = (np.asarray(tri[k], f32) for k in range(3))
        e1, e2 = v1 - v0, v2 - v0
        n = _cross(e1, e2)
        o, d, tmin, tmax = np.asarray(ray[0:3], f32), np.asarray(ray[4:7], f32), f32(ray[3]), f32(ray[7])
        tvec = o - v0
        q = _cross(tvec, d)
        det = -_dot(d, n)
        U, V, T = _dot(e2, q), -_dot(e1, q), _dot(tvec, n)
        if det < 0:
            U, V, T, det = -U, -V, -T, -det
        return bool(det > 0 and U >= 0 and V >= 0 and U + V <= det and T > tmin * det and T < tmax * det)


def filtered_occlusion(ray, tris, mesh_of_tri, masks, cull=None, mask=None, cands=None, slack=1e-5):
    """1 when some triangle that passes the filters satisfies the occlusion form, else 0.  The exact test runs on the triangles the
    oracle's divided test accepts on an interval widened by `slack` (relative): the two forms differ only where T / det rounds
    across an interval end, so those are a superset of the occluders."""
    wide = np.array(ray, f32)
    with np.errstate(all="ignore"):
        wide[3] = f32(ray[3]) - f32(slack) * (f32(1) + abs(f32(ray[3])))
        if np.isfinite(ray[7]):
            wide[7] = f32(ray[7]) + f32(slack) * (f32(1) + abs(f32(ray[7])))
    for *_, g in all_hits(wide, tris, cands):
        if keep(facing(ray, tris[g]), 0xFF if masks is None else masks[mesh_of_tri[g]], cull, mask) and occludes(ray, tris[g]):
            return 1
    return 0


def keep(hit_facing, mesh_mask, cull, mask):
    """does a triangle of that facing and mesh mask pass cull (None | "back" | "front") and the inclusion mask (None = 0xFF)?"""
    if cull == "back" and hit_facing < 0:
        return False
    if cull == "front" and hit_facing > 0:
        return False
    return (int(mesh_mask) & (0xFF if mask is None else int(mask)) & 0xFF) != 0


def faced_hits(ray, tris, cands=None):
    """all_hits with each hit's facing appended: (t, u, v, id, facing)"""
    return [h + (facing(ray, tris[h[3]]),) for h in all_hits(ray, tris, cands)]


def filtered_hits(ray, tris, mesh_of_tri, masks, cull=None, mask=None, cands=None, faced=None):
    """The filtered hit set in (t, id) order as (t, u, v, id): every hit of the contract (the oracle's triangle test, all_hits)
    whose triangle passes the cull and whose mesh's mask meets the inclusion mask.  masks=None: every mesh 0xFF.  faced: the
    result of faced_hits(ray, tris, cands), to filter one brute force several ways."""
    if faced is None:
        faced = faced_hits(ray, tris, cands)
    return [h[:4] for h in faced if keep(h[4], 0xFF if masks is None else masks[mesh_of_tri[h[3]]], cull, mask)]


def closest_record(hits, tmax):
    """the CapHit of a hit list: its first entry, or the miss record"""
    return records(hits, 1, tmax)[0]


def mesh_of_triangles(meshes):
    """mesh index per global triangle id from a (M, 8) mesh table"""
    m = np.asarray(meshes, np.uint32).reshape(-1, 8)
    return np.repeat(np.arange(len(m)), m[:, 2].astype(np.int64) // 3)


def stacked_quads_meshes(n=40, dz=0.25, flip_every=0):
    """multi_hit_support.stacked_quads with one mesh per quad: quad i (plane z = i * dz, normal e1 x e2 = +z) is mesh i with the
    triangles 2i (y <= x) and 2i + 1 (y >= x).  flip_every = f > 0 winds the quads with i % f == f - 1 the other way (v1 and v2 of
    both triangles swapped, e1 x e2 = -z), so that a vertical ray meets both facings.  Returns (positions, normals, texcoords,
    indices, meshes) and the (2n, 3, 3) triangles in global id order."""
    P, I, M = [], [], []
    for i in range(n):
        z = i * dz
        M.append([4, len(P), 6, len(I), i, 0xFFFFFFFF, 0, 0])
        P += [(0, 0, z), (1, 0, z), (1, 1, z), (0, 1, z)]
        flip = flip_every > 0 and i % flip_every == flip_every - 1
        I += [0, 2, 1, 0, 3, 2] if flip else [0, 1, 2, 0, 2, 3]  # indices are relative to the mesh's first vertex
    P = np.array(P, f32)
    I = np.array(I, np.uint32)
    N = np.tile(f32([0, 0, 1]), (len(P), 1))
    T = np.zeros((len(P), 2), f32)
    tris = np.stack([P[4 * (g // 2) + I[3 * g:3 * g + 3].astype(np.int64)] for g in range(2 * n)])
    return (P, N, T, I, np.array(M, np.uint32)), tris.astype(f32)
