"""Helpers of the instanced winding-number tests (cap_winding_instances): the float64 brute force over the flattened world triangles,
the float64 definition of the derived tables of include/capsaicin_hip.h ("winding numbers over instances"), and the two-level walk
restated on the host from the read-backs -- every decision in float32 exactly as the header writes it, the terms in float64 on the world
triangles (walk) or in the kernel's float32 forms (walk32).  The CPU tests build the same tables on the host (host_state) over
winding_support.median_tree, so both run the same walk code."""
import numpy as np

from signed_distance_support import winding_number
from winding_support import K4PI, KINV2PI, _dot, _records32, leaf_range, median_tree, moments, root_code, table32_of, triangle_sums

f32 = np.float32
EMPTY = 0xFFFFFFFF


# ---- the flattened scene, float64 ----
def linear(M):
    return np.asarray(M, f32).astype(np.float64).reshape(-1, 3, 4)[:, :, 0:3]


def contributes(M, masks, live):
    """instance i contributes iff it is not inert, its mask is not 0 and det L is a finite number other than 0"""
    det = np.linalg.det(linear(M))
    return np.asarray(live, bool) & ((np.asarray(masks).astype(np.int64) & 0xFF) != 0) & np.isfinite(det) & (det != 0)


def world_triangles(M, on, tris, ranges=None, objects=None):
    """(K, 3, 3) float64: the triangles of every contributing instance under its transform, vertex order swapped under a mirror (that
    swap is s_i).  ranges: (first triangle, count) per object, objects: the object of every instance; None: the whole scene"""
    M = np.asarray(M, f32).astype(np.float64).reshape(-1, 3, 4)
    t = np.asarray(tris, f32).astype(np.float64).reshape(-1, 3, 3)
    out = []
    for i in np.nonzero(on)[0]:
        mine = t if ranges is None else t[ranges[objects[i]][0]:ranges[objects[i]][0] + ranges[objects[i]][1]]
        w = mine @ M[i, :, 0:3].T + M[i, :, 3]
        out.append(w[:, [0, 2, 1]] if np.linalg.det(M[i, :, 0:3]) < 0 else w)
    return np.concatenate(out) if out else np.zeros((0, 3, 3))


def brute_force(points, M, on, tris, ranges=None, objects=None):
    """the definition: the float64 winding number of the flattened world scene"""
    w = world_triangles(M, on, tris, ranges, objects)
    return winding_number(points, w) if len(w) else np.zeros(len(points))


# ---- the derived tables, float64 ----
def instance_records(M, on):
    """(I, 12) float64: L, |det L|, sigma = sqrt(||L||_1 ||L||_inf) (not yet rounded up), s"""
    L = linear(M)
    out = np.zeros((len(L), 12))
    out[:, 0:9] = L.reshape(-1, 9)
    det = np.linalg.det(L)
    out[:, 9] = np.abs(det)
    out[:, 10] = np.sqrt(np.abs(L).sum(1).max(1) * np.abs(L).sum(2).max(1))
    out[:, 11] = np.where(on, np.where(det < 0, -1.0, 1.0), 0.0)
    return out


def cofactor(L):
    return np.stack([np.cross(L[1], L[2]), np.cross(L[2], L[0]), np.cross(L[0], L[1])])


def level_offsets(level_entries):
    n = [int(x) for x in level_entries if int(x)]
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64), len(n)


def top_moments(M, on, order0, obj_sums, boxes, level_entries):
    """(table (entries, 8) float64 = p~_w, r, N_w, word 7; dict of per-entry weight, stored box lo / hi, and nbound >= |N_w| the sum
    of ||cof L||_F A over the instances below) of the definition.  order0: the instance of every level-0
    entry (EMPTY for the padding), obj_sums: (I, 7) the root sums (N, A, M) of each instance's object, boxes: (I, 2, 3) the stored
    world boxes.  p~_w and N_w are not yet rounded; r is measured from the float32-rounded p~_w, not yet rounded or stepped."""
    M = np.asarray(M, f32).astype(np.float64).reshape(-1, 3, 4)
    off, levels = level_offsets(level_entries)
    total = int(off[-1])
    sums, lo, hi = np.zeros((total, 7)), np.full((total, 3), np.inf), np.full((total, 3), -np.inf)
    full, word7, nbound = np.zeros(total, bool), np.full(total, EMPTY, np.int64), np.zeros(total)
    for j, i in enumerate(order0):
        word7[j] = i
        if i == EMPTY:
            continue
        lo[j], hi[j] = boxes[i, 0], boxes[i, 1]
        if not on[i]:
            continue
        L, o = M[i, :, 0:3], obj_sums[i]
        det = np.linalg.det(L)
        w = o[3] * np.cbrt(det * det)
        p = M[i, :, 0:3] @ (o[4:7] / o[3]) + M[i, :, 3] if o[3] != 0 else np.zeros(3)
        sums[j, 0:3], sums[j, 3], sums[j, 4:7] = np.sign(det) * (cofactor(L) @ o[0:3]), w, w * p
        full[j], nbound[j] = True, np.linalg.norm(cofactor(L)) * o[3]
    for l in range(1, levels):
        for j in range(int(level_entries[l])):
            a, b, me = off[l - 1] + 2 * j, off[l - 1] + 2 * j + 1, off[l] + j
            if b >= off[l]:
                continue  # (the padding entry of this level)
            sums[me], full[me], nbound[me] = sums[a] + sums[b], full[a] or full[b], nbound[a] + nbound[b]
            lo[me], hi[me] = np.minimum(lo[a], lo[b]), np.maximum(hi[a], hi[b])
    table = np.zeros((total, 8))
    table[:, 3], table[:, 7] = -1.0, word7
    for e in np.nonzero(full)[0]:
        p = sums[e, 4:7] / sums[e, 3] if sums[e, 3] != 0 else 0.5 * (lo[e] + hi[e])
        p32 = p.astype(f32).astype(np.float64)
        d = np.maximum(np.abs(lo[e] - p32), np.abs(hi[e] - p32))
        table[e, 0:3], table[e, 3], table[e, 4:7] = p, np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), sums[e, 0:3]
    return table, dict(weight=sums[:, 3], lo=lo, hi=hi, nbound=nbound, full=full)


def top32_of(table64):
    """the float32 table the device would store: p~_w and N_w rounded once, r rounded and stepped one ulp up (-1 stays), word 7's bits"""
    t = np.zeros(table64.shape, f32)
    t[:, 0:3], t[:, 4:7] = table64[:, 0:3], table64[:, 4:7]
    r = table64[:, 3].astype(f32)
    t[:, 3] = np.where(r >= 0, np.nextafter(r, f32(np.inf)), r)
    t.view(np.uint32)[:, 7] = table64[:, 7].astype(np.int64).astype(np.uint32)
    return t


def inst32_of(rec64):
    """the float32 per-instance records: every word rounded once, sigma rounded UP"""
    t = rec64.astype(f32)
    s = t[:, 10]
    t[:, 10] = np.where(s.astype(np.float64) < rec64[:, 10], np.nextafter(s, f32(np.inf)), s)
    return t


# ---- the walk ----
class State:
    """What the walk reads: top (entries, 8) float32 and level_entries, inst (I, 12) float32, W (I, 3, 4) float32, roots (I,) the root
    code of every instance's object tree, table32 (nodes, 2, 8) the objects' dipole table, order the triangle of every leaf-order
    record, tris (T, 3, 3), M (I, 3, 4) the descriptors (walk's float64 terms are taken on the world triangles M t)"""

    def __init__(self, top, level_entries, inst, W, roots, table32, order, tris, M):
        self.top, self.level_entries = np.asarray(top, f32).reshape(-1, 8), [int(x) for x in level_entries]
        self.inst, self.W, self.roots = np.asarray(inst, f32).reshape(-1, 12), np.asarray(W, f32).reshape(-1, 3, 4), [int(x) for x in roots]
        self.table32, self.order = np.asarray(table32, f32).reshape(-1, 2, 8), np.asarray(order).astype(np.int64)
        self.tris, self.M = np.asarray(tris, f32).reshape(-1, 3, 3), np.asarray(M, f32).reshape(-1, 3, 4)


def _exact64(q, tri):
    a, b, c = (tri[k][None] - q for k in range(3))
    la, lb, lc = (np.sqrt((x * x).sum(1)) for x in (a, b, c))
    num = (a * np.cross(b, c)).sum(1)
    den = la * lb * lc + (a * b).sum(1) * lc + (b * c).sum(1) * la + (c * a).sum(1) * lb
    return 2.0 * np.arctan2(num, den) / (4.0 * np.pi)


def _to_world32(L, d):
    """d_w = (dot(L_0, d'), dot(L_1, d'), dot(L_2, d')) in float32"""
    return np.stack([_dot(L[r][None], d) for r in range(3)], 1)


def _walk(st, points, beta, single):
    q32 = np.ascontiguousarray(np.asarray(points, f32)[:, 0:3])
    q64 = q32.astype(np.float64)
    N = len(q32)
    acc, visits = np.zeros(N), np.zeros((N, 4), np.int64)
    ok = np.isfinite(q32).all(1)
    beta = f32(beta)
    off, levels = level_offsets(st.level_entries)
    word7 = st.top.view(np.uint32)[:, 7]
    codes = st.table32.view(np.int32)[:, :, 7] if len(st.table32) else None
    rec = _records32(st.tris, st.order)
    t64 = st.tris.astype(np.float64)[st.order]

    def add(idx, term):
        acc[idx] += np.where(np.isnan(term), 0.0, term)

    def instance(i, idx):
        W, L32, det, sigma = st.W[i], st.inst[i, 0:9].reshape(3, 3), st.inst[i, 9], st.inst[i, 10]
        p = np.stack([((W[r, 0] * q32[idx, 0] + W[r, 1] * q32[idx, 1]) + W[r, 2] * q32[idx, 2]) + W[r, 3] for r in range(3)], 1)
        assert p.dtype == f32
        good = np.isfinite(p).all(1)
        idx, p = idx[good], p[good]
        visits[idx, 1] += 1
        M64 = st.M[i].astype(np.float64)
        L64 = M64[:, 0:3]
        s = -1.0 if np.linalg.det(L64) < 0 else 1.0
        cof = cofactor(L64)
        stack = [(st.roots[i], idx, p)]
        while stack:
            code, ids, pp = stack.pop()
            if len(ids) == 0:
                continue
            if code < 0:
                first, end = leaf_range(code)
                for t in range(first, end):
                    if single:
                        a = rec[0][t][None] - pp
                        b, c = a + rec[1][t][None], a + rec[2][t][None]
                        aw, bw, cw = _to_world32(L32, a), _to_world32(L32, b), _to_world32(L32, c)
                        la, lb, lc = np.sqrt(_dot(aw, aw)), np.sqrt(_dot(bw, bw)), np.sqrt(_dot(cw, cw))
                        dt = det * _dot(a, rec[3][t][None])
                        den = (((la * lb) * lc + _dot(aw, bw) * lc) + _dot(bw, cw) * la) + _dot(cw, aw) * lb
                        term = np.arctan2(dt, den) * KINV2PI
                        assert term.dtype == f32
                        term = term.astype(np.float64)
                    else:
                        term = s * _exact64(q64[ids], t64[t] @ L64.T + M64[:, 3])
                    add(ids, term)
                visits[ids, 3] += end - first
                continue
            near = []
            for slot in range(2):
                pc, r, nn = st.table32[code, slot, 0:3], st.table32[code, slot, 3], st.table32[code, slot, 4:7]
                d = pc[None] - pp
                dw = _to_world32(L32, d)
                d2 = _dot(dw, dw)
                lim = beta * (sigma * r)
                far = d2 > lim * lim
                assert d2.dtype == f32 and np.asarray(lim).dtype == f32
                if single:
                    term = ((det * _dot(nn[None], d)) / ((K4PI * d2) * np.sqrt(d2))).astype(np.float64)
                else:
                    dw64 = (M64[:, 0:3] @ pc.astype(np.float64) + M64[:, 3])[None] - q64[ids]
                    l2 = (dw64 * dw64).sum(1)
                    term = (s * (cof @ nn.astype(np.float64))[None] * dw64).sum(1) / (4.0 * np.pi * l2 * np.sqrt(l2))
                add(ids[far], term[far])
                visits[ids[far], 2] += 1
                near.append((ids[~far], pp[~far]))
            stack.append((int(codes[code, 1]),) + near[1])
            stack.append((int(codes[code, 0]),) + near[0])

    def node(level, j, idx):
        """the node whose two entries are (level - 1, 2 j + {0, 1})"""
        near = []
        for slot in range(2):
            e = st.top[off[level - 1] + 2 * j + slot]
            if not e[3] >= 0:
                near.append(idx[:0])
                continue
            d = e[0:3][None] - q32[idx]
            d2 = _dot(d, d)
            lim = beta * e[3]
            far = d2 > lim * lim
            assert d2.dtype == f32 and np.asarray(lim).dtype == f32
            if single:
                term = (_dot(e[4:7][None], d) / ((K4PI * d2) * np.sqrt(d2))).astype(np.float64)
            else:
                d64 = e[0:3].astype(np.float64)[None] - q64[idx]
                l2 = (d64 * d64).sum(1)
                term = (e[4:7].astype(np.float64)[None] * d64).sum(1) / (4.0 * np.pi * l2 * np.sqrt(l2))
            add(idx[far], term[far])
            visits[idx[far], 0] += 1
            near.append(idx[~far])
        for slot in range(2):
            if len(near[slot]) == 0:
                continue
            if level > 1:
                node(level - 1, 2 * j + slot, near[slot])
            else:
                instance(int(word7[off[0] + 2 * j + slot]), near[slot])

    with np.errstate(all="ignore"):
        if levels and len(st.tris):
            node(levels, 0, np.nonzero(ok)[0])
    acc[~ok] = np.nan
    return acc, visits


def walk(st, points, beta):
    """(w (N,) float64, visits (N, 4)) of cap_winding_instances' walk over the State: the decisions in float32 as specified, the far
    terms in float64 on the stored world dipoles, the exact terms in float64 on the world triangles"""
    return _walk(st, points, beta, False)


def walk32(st, points, beta):
    """the same walk with every term in the kernel's float32 arithmetic, widened and added into a float64 accumulator"""
    return _walk(st, points, beta, True)


# ---- the state without a device (the CPU tests) ----
def host_state(tris, M, masks=None, ranges=None, objects=None, leaf=4):
    """(State, on) built on the host: a median tree per object (the whole scene without ranges), the float32 roundings of the float64
    tables, W = the float32 rounding of the float64 inverse, world boxes = the bounds of the transformed vertices, level 0 in the
    instances' own order"""
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    M = np.asarray(M, f32).reshape(-1, 3, 4)
    I = len(M)
    masks = np.full(I, 0xFF) if masks is None else np.asarray(masks)
    on = contributes(M, masks, np.ones(I, bool))
    if ranges is None:
        ranges, objects = [(0, len(tris))], np.zeros(I, np.int64)
    nodes_all, order_all, roots_of, sums_of = [], [], [], []
    nb = rb = 0
    for first, count in ranges:
        mine = tris[first:first + count]
        nodes, order = median_tree(mine, leaf)
        kid = nodes.view(np.int32)
        for col in (12, 13, 14, 15):  # the forest's numbering
            c = kid[:, col].astype(np.int64)
            inner = c >= 0
            code = ~c[~inner]
            kid[inner, col] = (c[inner] + nb).astype(np.int32)
            kid[~inner, col] = (~(((code & ((1 << 27) - 1)) + rb) | (code & ~((1 << 27) - 1)))).astype(np.int32)
        roots_of.append(nb if count >= 2 else ~rb)
        sums_of.append(triangle_sums(mine)[0].sum(0))
        nodes_all.append(nodes), order_all.append(order.astype(np.int64) + first)
        nb, rb = nb + max(count - 1, 0), rb + count
    nodes, order = np.concatenate(nodes_all), np.concatenate(order_all)
    table32 = table32_of(moments(nodes, order, tris)[0]) if len(nodes) else np.zeros((0, 2, 8), f32)
    M64 = M.astype(np.float64)
    W = np.zeros((I, 3, 4), f32)
    boxes = np.zeros((I, 2, 3))
    for i in range(I):
        inv = np.linalg.inv(M64[i, :, 0:3])
        W[i, :, 0:3], W[i, :, 3] = inv, -inv @ M64[i, :, 3]
        first, count = ranges[objects[i]]
        v = tris[first:first + count].reshape(-1, 3).astype(np.float64) @ M64[i, :, 0:3].T + M64[i, :, 3]
        boxes[i] = v.min(0) - 1e-4, v.max(0) + 1e-4
    level_entries, cnt = [], I
    while True:
        level_entries.append(cnt + (cnt & 1))
        if cnt <= 1:
            break
        cnt = (cnt + 1) // 2
    order0 = list(range(I)) + [EMPTY] * (I & 1)
    obj_sums = np.stack([sums_of[objects[i]] for i in range(I)])
    top = top32_of(top_moments(M, on, order0, obj_sums, boxes.astype(f32).astype(np.float64), level_entries)[0])
    inst = inst32_of(instance_records(M, on))
    return State(top, level_entries, inst, W, [roots_of[objects[i]] for i in range(I)], table32, order, tris, M), on


# ---- transforms ----
def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def affine(L, t):
    m = np.zeros((3, 4), f32)
    m[:, 0:3], m[:, 3] = L, t
    return m


IDENTITY = affine(np.eye(3), (0, 0, 0))


def grid_transforms(n, pitch=3.0, seed=4, centre=(0.5, 0.5, 0.5)):
    """n^3 transforms on a grid of that pitch: rotation x diag(0.5 .. 1.5) about `centre`, every third one mirrored"""
    rng = np.random.default_rng(seed)
    out, c = [], np.float64(centre)
    for k in range(n ** 3):
        L = rotation(rng) @ np.diag(rng.uniform(0.5, 1.5, 3))
        if k % 3 == 2:
            L = L @ np.diag([1.0, 1.0, -1.0])
        at = pitch * np.float64([k % n, (k // n) % n, k // (n * n)])
        out.append(affine(L, at + c - L @ c))
    return np.stack(out)


def points_about(rng, M, on, tris, n, grow=0.5, ranges=None, objects=None):
    """(n, 4) float32 queries uniform in the bounds of the flattened scene grown by `grow`"""
    w = world_triangles(M, on, tris, ranges, objects).reshape(-1, 3)
    q = np.zeros((n, 4), f32)
    q[:, 0:3], q[:, 3] = rng.uniform(w.min(0) - grow, w.max(0) + grow, (n, 3)), np.inf
    return q


def off_surface(q, M, on, tris, ranges=None, objects=None, rel=1e-3):
    """the points at least `rel` of an object's diagonal (the smallest object's) off the flattened scene's surface: on it a term jumps
    by 1/2 with a rounding error.  (Not of the flattened scene's diagonal: an instance placed 4096 away would make that everything.)"""
    from closest_point_support import closest
    t = np.asarray(tris, f32).astype(np.float64).reshape(-1, 3, 3)
    parts = [t] if ranges is None else [t[f:f + c] for f, c in ranges]
    diag = min(np.linalg.norm(x.reshape(-1, 3).max(0) - x.reshape(-1, 3).min(0)) for x in parts)
    rec, _ = closest(q, world_triangles(M, on, tris, ranges, objects).astype(f32))
    return np.sqrt(rec[:, 3].astype(np.float64)) >= rel * diag
