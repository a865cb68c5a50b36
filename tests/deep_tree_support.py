"""Helpers of the deep-tree tests: a 3-axis geometric spiral of n triangles that the host SAH builder peels one triangle per level
(depth n - 2 for n in 16 .. 40), model walkers of the binary tree for rays and points in the kernels' own float32 operations -- they
report how many stack entries a walk holds at once and which entry the answer came out of --, and the fixed query sets of the tests."""
import numpy as np

from closest_point_support import arrays, queries
from instance_support import degenerate_rays

f32 = np.float32
LEAF_SHIFT, LEAF_MASK = 27, (1 << 27) - 1
RATIO = 2.5
SIZES = (18, 19, 26, 27, 34, 35, 40)  # depths 16, 17, 24, 25, 32, 33, 38: both sides of every stack size class
BY_DESCENT = -1  # the slot of an answer no stack entry lies on the way to


def depth_of(n):
    """the host SAH builder's depth on the spiral of n triangles, 16 <= n <= 40"""
    return n - 2


def scales(n):
    return RATIO ** (np.arange(n) - (n - 1) / 2.0)


def spiral(n):
    """(n, 3, 3) float32: triangle k has the centre s_k e_(k mod 3), s_k = 2.5^(k - (n - 1) / 2), and the vertices centre + 1.5 s_k
    {(-1, -1, 1), (1, -1, -1), (-1, 1, -1)}.  Every triangle's box contains the neighbourhood of the origin."""
    s = scales(n)
    c = np.zeros((n, 3))
    c[np.arange(n), np.arange(n) % 3] = s
    off = np.array([(-1.0, -1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0)])
    return (c[:, None, :] + 1.5 * s[:, None, None] * off[None]).astype(f32)


def spiral_arrays(tris):
    """GeometryStorage arrays (positions, normals, texcoords, indices, meshes), one mesh per triangle"""
    return arrays(*[t[None] for t in tris])


def mesh_masks(n):
    """mesh k carries the mask 1 << (k % 8)"""
    return (1 << (np.arange(n) % 8)).astype(np.uint8)


def tri_boxes(tris):
    return tris.min(1), tris.max(1)


# ---- the model walkers ----
def _children(nodes):
    return np.ascontiguousarray(nodes[:, 14:16]).view(np.int32)


def _leaf_range(code_node):
    code = ~int(code_node) & 0xFFFFFFFF
    first = code & LEAF_MASK
    return range(first, first + (code >> LEAF_SHIFT) + 1)


def _slab(o, inv, tmin, lo, hi, tfar):
    """cap_trace.h slab(): float32 throughout, fminf / fmaxf drop a NaN"""
    with np.errstate(all="ignore"):
        a, b = (lo - o) * inv, (hi - o) * inv
        near, far = np.fmin(a, b), np.fmax(a, b)
        tn = np.fmax(np.fmax(near[0], near[1]), np.fmax(near[2], tmin))
        tf = np.fmin(np.fmin(far[0], far[1]), np.fmin(far[2], tfar))
        return bool(tn <= tf * f32(1.0000004)), tn


def ray_walk(nodes, order, tris, ray):
    """k_query_binary_f's closest-hit walk of one ray: both children hit -> descend the nearer one (child 0 on a tie) and push the
    other, best_t shrinking.  Returns (stack high-water, winning triangle or None, the highest stack slot on the way to the winner's
    leaf or BY_DESCENT, number of triangles tested)."""
    from oracle import cap_oracle as O
    ray = np.asarray(ray, f32)
    o, d, tmin = ray[0:3], ray[4:7], ray[3]
    with np.errstate(all="ignore"):
        inv = f32(1.0) / d
    kid = _children(nodes)
    best_t, best_g, best_slot = ray[7], None, BY_DESCENT
    stack, high, tested = [], 0, 0
    node, slot = 0, BY_DESCENT
    while True:
        if node >= 0:
            q = nodes[node]
            h0, tn0 = _slab(o, inv, tmin, q[0:3], q[3:6], best_t)
            h1, tn1 = _slab(o, inv, tmin, q[6:9], q[9:12], best_t)
            c0, c1 = int(kid[node, 0]), int(kid[node, 1])
            if h0 and h1:
                swap = bool(tn1 < tn0)
                stack.append((c0 if swap else c1, slot))
                high = max(high, len(stack))
                node = c1 if swap else c0
                continue
            if h0 or h1:
                node = c0 if h0 else c1
                continue
        else:
            for leaf in _leaf_range(node):
                g = int(order[leaf])
                tested += 1
                h = O.intersect_triangle(o, d, float(tmin), float(ray[7]), tris[g, 0], tris[g, 1], tris[g, 2])
                if h is None:
                    continue
                t = f32(h[0])
                if t < best_t or (t == best_t and (best_g is None or g < best_g)):
                    best_t, best_g, best_slot = t, g, slot
        if not stack:
            break
        node, pushed_under = stack.pop()
        slot = max(pushed_under, len(stack))
    return high, best_g, best_slot, tested


def _box_dist2(p, lo, hi):
    d = np.maximum(np.maximum(lo - p, p - hi), f32(0))
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def _prune_bound2(best, slack):
    with np.errstate(all="ignore"):
        b = np.sqrt(f32(best)) * (f32(1.0) + f32(16.0) * f32(5.9604645e-8)) + slack
        return (b * b) * (f32(1.0) + f32(4.0) * f32(5.9604645e-8))


def closest_slack(tris):
    """the absolute part of the pruning bound as the launcher computes it: 2^-18 x max(scene extent, largest |coordinate|)"""
    lo, hi = tris.reshape(-1, 3).min(0).astype(np.float64), tris.reshape(-1, 3).max(0).astype(np.float64)
    return f32(max((hi - lo).max(), np.abs(lo).max(), np.abs(hi).max()) / 262144.0)


def point_walk(nodes, order, tris, query, table):
    """k_closest_points' walk of one query (x, y, z, radius): both children within the bound -> descend the nearer box (child 0 on a
    tie) and push the other with its distance, which is tested again on the pop.  table: this query's row of the float32 dist2 table
    of closest_point_support.closest.  Returns (stack high-water, winning triangle or None, highest slot on the way, triangles tested)."""
    q = np.asarray(query, f32)
    p = q[0:3]
    slack = closest_slack(tris)
    with np.errstate(all="ignore"):
        best = q[3] * q[3]
    bound2 = _prune_bound2(best, slack)
    kid = _children(nodes)
    best_g, best_slot = None, BY_DESCENT
    stack, high, tested = [], 0, 0
    node, slot = 0, BY_DESCENT
    while True:
        if node >= 0:
            n_ = nodes[node]
            b0, b1 = _box_dist2(p, n_[0:3], n_[3:6]), _box_dist2(p, n_[6:9], n_[9:12])
            c0, c1 = int(kid[node, 0]), int(kid[node, 1])
            k0, k1 = not b0 > bound2, not b1 > bound2
            if k0 and k1:
                swap = bool(b1 < b0)
                stack.append((b0 if swap else b1, c0 if swap else c1, slot))
                high = max(high, len(stack))
                node = c1 if swap else c0
                continue
            if k0 or k1:
                node = c0 if k0 else c1
                continue
        else:
            for leaf in _leaf_range(node):
                g = int(order[leaf])
                tested += 1
                d2 = table[g]
                if d2 < best or (d2 == best and (best_g is None or g < best_g)):
                    if d2 < best:
                        bound2 = _prune_bound2(d2, slack)
                    best, best_g, best_slot = d2, g, slot
        more = False
        while stack:
            b, c, pushed_under = stack.pop()
            if not b > bound2:
                node, slot, more = c, max(pushed_under, len(stack)), True
                break
        if not more:
            break
    return high, best_g, best_slot, tested


# ---- the query sets ----
def _rays(o, d, tmin=0.0, tmax=np.inf):
    o, d = np.atleast_2d(np.asarray(o, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
    r = np.zeros((max(len(o), len(d)), 8), f32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64)


def ray_set(n, seed=2024, with_degenerate=True):
    """The rays of the tests, fixed by the seed (about 190): random origins within 0.01 s_0 of the origin with random directions, the
    same origins along the six axes (zero components), rays from outside the largest triangle at the origin, rays from each centroid
    outward, a finite tmax that cuts the chain in the middle, a tmin past the first few hits, and the degenerate rays."""
    rng = np.random.default_rng(seed + n)
    s = scales(n)
    tris = spiral(n).astype(np.float64)
    o = rng.uniform(-1, 1, (48, 3)) * 0.01 * s[0]
    d = _unit(rng.normal(size=(48, 3)))
    parts = [_rays(o, d)]
    parts.append(_rays(np.repeat(o[:4], 6, axis=0), np.tile(AXES, (4, 1))))
    far = _unit(rng.normal(size=(24, 3))) * 8.0 * s[-1]
    parts.append(_rays(far, -far + rng.uniform(-1, 1, (24, 3)) * 0.01 * s[0]))
    cen = tris.mean(1)
    parts.append(_rays(cen * 0.999, _unit(cen)))
    parts.append(_rays(cen * 0.5, -_unit(cen)))
    mid = s[n // 2]
    parts.append(_rays(o[:16], d[:16], 0.0, 0.6 * mid))
    parts.append(_rays(o[16:32], d[16:32], 0.3 * s[3], np.inf))
    parts.append(_rays(o[32:40], d[32:40], 0.3 * s[2], 0.8 * mid))
    if with_degenerate:
        parts.append(degenerate_rays())
    return np.concatenate(parts).astype(f32)


def point_set(n, seed=4048):
    """The closest-point queries of the tests, fixed by the seed (about 170): random points at 0.01, 0.3, 1 and 3 times s_0, each
    triangle's centroid; radius infinity, radius 0, and a radius that excludes some triangles."""
    rng = np.random.default_rng(seed + n)
    s = scales(n)
    tris = spiral(n).astype(np.float64)
    xyz = [rng.uniform(-1, 1, (24, 3)) * m * s[0] for m in (0.01, 0.3, 1.0, 3.0)]
    xyz.append(tris.mean(1))
    xyz = np.concatenate(xyz)
    q = queries(xyz)
    some = queries(xyz[::4], 0.0)
    near = queries(xyz[1::4])
    near[:, 3] = (np.linalg.norm(xyz[1::4], axis=1) + 0.2 * s[np.arange(len(near)) % n]).astype(f32)  # only part of the chain is within it
    return np.concatenate([q, some, near]).astype(f32)
