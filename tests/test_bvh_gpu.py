"""On-device LBVH: structural invariants of the built tree and traversal parity on scenes other than the Cornell box."""
import numpy as np
import pytest

from capsaicin_amd import capi

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, ref, name):
    g, r = bits(got), bits(ref)
    if not np.array_equal(g, r):
        bad = np.argwhere((g != r).any(-1))
        msg = ["%s: %d pixels differ" % (name, len(bad))]
        for b in bad[:6]:
            msg.append("  (y,x)=%s gpu=%s oracle=%s" % (tuple(b), got[tuple(b)], ref[tuple(b)]))
        raise AssertionError("\n".join(msg))


def soup(seed, ntri, spread=2.0, size=0.8):
    rs = np.random.RandomState(seed)
    c = rs.rand(ntri, 1, 3) * 2 * spread - spread
    v = (c + (rs.rand(ntri, 3, 3) - 0.5) * size).astype(np.float32)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-20)
    nrm = np.repeat(n[:, None, :], 3, axis=1).reshape(-1, 3).astype(np.float32)
    uv = rs.rand(ntri * 3, 2).astype(np.float32)
    idx = np.arange(ntri * 3, dtype=np.uint32)
    cut = (ntri // 3) * 3
    meshes = np.array([[cut, 0, cut, 0, 0, 0xFFFFFFFF, 0, 0], [ntri * 3 - cut, cut, ntri * 3 - cut, cut, 1, 0xFFFFFFFF, 0, 0]], np.uint32)
    idx[cut:] -= cut
    if cut == 0 or cut == ntri * 3:
        meshes = np.array([[ntri * 3, 0, ntri * 3, 0, 0, 0xFFFFFFFF, 0, 0]], np.uint32)
        idx = np.arange(ntri * 3, dtype=np.uint32)
    return v.reshape(-1, 3), nrm, uv, idx, meshes


def check_tree(nodes, leaves, tri_lo, tri_hi):
    n = len(leaves)
    assert sorted(leaves.tolist()) == list(range(n))
    if n < 2:
        return 0
    child = nodes[:, 12:14].copy().view(np.int32)
    seen_nodes, seen_leaves = np.zeros(n - 1, bool), np.zeros(n, bool)
    max_depth = 0

    def box_of(c):
        if c < 0:
            g = leaves[~c]
            return tri_lo[g], tri_hi[g]
        q = nodes[c]
        return np.minimum(q[0:3], q[6:9]), np.maximum(q[3:6], q[9:12])

    stack = [(0, 1)]
    while stack:
        i, d = stack.pop()
        assert not seen_nodes[i]
        seen_nodes[i] = True
        max_depth = max(max_depth, d)
        q = nodes[i]
        for slot, c in enumerate(child[i]):
            lo, hi = (q[0:3], q[3:6]) if slot == 0 else (q[6:9], q[9:12])
            clo, chi = box_of(int(c))
            # the stored child box contains the child's content (leaf boxes are padded, so >=)
            assert np.all(lo <= clo + 1e-30) and np.all(hi >= chi - 1e-30), (i, slot)
            if c < 0:
                assert not seen_leaves[~c]
                seen_leaves[~c] = True
                pad = 1e-4 * np.maximum(1.0, np.maximum(np.abs(clo), np.abs(chi)))
                assert np.all(lo >= clo - pad) and np.all(hi <= chi + pad)  # ... and is tight
            else:
                stack.append((int(c), d + 1))
    assert seen_nodes.all() and seen_leaves.all()
    return max_depth


# on-device LBVH, host-side SAH, on-device clustering, on-device SAH: same layout, same invariants; the device builders also past one
# scan tile of the radix sort's histogram (32768 triangles) and into its third
INVARIANT_CASES = [(seed, ntri, build) for seed, ntri in [(1, 1), (2, 2), (3, 3), (4, 33), (5, 1000), (6, 20000)] for build in (1, 2, 3, 4)]
INVARIANT_CASES += [(seed, ntri, build) for seed, ntri in [(7, 32769), (8, 65537)] for build in (1, 3, 4)]


@pytest.mark.parametrize("seed,ntri,build", INVARIANT_CASES)
def test_lbvh_invariants(native_lib, bluenoise, seed, ntri, build):
    pos, nrm, uv, idx, meshes = soup(seed, ntri)
    r = capi.Renderer(0)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    r.set_bvh_build(build)
    info = r.build_bvh()
    assert info.triangle_count == ntri and info.node_count == max(0, ntri - 1)
    nodes, leaves = r.bvh_readback()
    tri = pos.reshape(-1, 3, 3)
    depth = check_tree(nodes, leaves, tri.min(1), tri.max(1))
    assert depth == info.max_depth and info.stack_entries >= info.max_depth
    np.testing.assert_array_equal(np.float32(info.bounds_lo), pos.min(0))
    np.testing.assert_array_equal(np.float32(info.bounds_hi), pos.max(0))
    r.close()


@pytest.mark.parametrize("build", [1, 2, 3, 4])
def test_identical_triangles(native_lib, bluenoise, build):
    # 3000 copies of one triangle: every Morton code, every box and every merge distance ties; the builders' index tie-breaks
    # must still produce a complete tree of bounded depth (the clustering build: mutual nearest neighbours exist in every round)
    n = 3000
    pos = np.tile(np.float32([[0.25, -1, 0.5], [1, 0.5, -0.25], [-0.5, 1, 2]]), (n, 1))
    r = capi.Renderer(0)
    r.upload_scene(pos, np.tile(np.float32([0, 0, 1]), (len(pos), 1)), np.zeros((len(pos), 2), np.float32),
                   np.arange(len(pos), dtype=np.uint32), np.uint32([[len(pos), 0, len(pos), 0, 0, 0xFFFFFFFF, 0, 0]]))
    r.set_bvh_build(build)
    info = r.build_bvh()
    nodes, leaves = r.bvh_readback()
    tri = pos.reshape(-1, 3, 3)
    assert check_tree(nodes, leaves, tri.min(1), tri.max(1)) == info.max_depth and info.max_depth <= 64
    r.close()


@pytest.mark.parametrize("build", [0, 1, 3, 4])
def test_duplicate_centroids_and_flat_scene(native_lib, bluenoise, build):
    # all triangles share one centroid / lie in one plane: Morton codes collide, the index tie-break must still give a tree
    base = np.float32([[-1, -1, 0], [1, -1, 0], [0, 2, 0]])
    pos = np.concatenate([base * s for s in (1.0, 0.5, 0.25, 2.0, 1.5, 0.75, 1.25)]).astype(np.float32)
    n = len(pos) // 3
    r = capi.Renderer(0)
    r.upload_scene(pos, np.tile(np.float32([0, 0, 1]), (len(pos), 1)), np.zeros((len(pos), 2), np.float32),
                   np.arange(len(pos), dtype=np.uint32), np.uint32([[len(pos), 0, len(pos), 0, 0, 0xFFFFFFFF, 0, 0]]))
    r.set_bvh_build(build)
    info = r.build_bvh()
    nodes, leaves = r.bvh_readback()
    tri = pos.reshape(-1, 3, 3)
    check_tree(nodes, leaves, tri.min(1), tri.max(1))
    assert info.node_count == n - 1
    r.close()


@pytest.mark.parametrize("build", [1, 2, 3, 4])
@pytest.mark.parametrize("seed,ntri,w,h,D", [(11, 1, 48, 48, 2), (12, 2, 48, 48, 2), (13, 300, 96, 96, 3), (14, 5000, 128, 96, 4),
                                            (15, 700, 61, 37, 3)])  # the last: partial tiles (idle lanes in the camera-ray packets)
def test_triangle_soup_parity(native_lib, bluenoise, seed, ntri, w, h, D, build):
    from oracle import cap_oracle as O
    pos, nrm, uv, idx, meshes = soup(seed, ntri)
    r = capi.Renderer(0)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    r.upload_bluenoise(bluenoise)
    r.set_bvh_build(build)
    r.build_bvh()
    cam = capi.CameraData()
    cam.position[:] = (0.3, 0.2, 6.0)
    cam.forward[:] = (0, 0, -1)
    cam.right[:] = (-1, 0, 0)
    cam.up[:] = (0, 1, 0)
    cam.focal_length = 0.03
    cam.sensor_size[0] = 0.036
    cam.sensor_size[1] = np.float32(0.036) * (np.float32(h) / np.float32(w))
    r.set_resolution(w, h)
    r.set_camera(cam)
    r.render(2, 1, D, capi.RENDER_AOV)
    sc = O.Scene(pos, nrm, uv, idx, meshes)
    ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1], cam.focal_length)
    ref = sc.render_frame(ocam, bluenoise, w, h, 2, D, flags=O.FLAG_USE_BVH if ntri > 500 else 0, threads=8)
    for name, kind in (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("direct", capi.BUF_DIRECT), ("indirect", capi.BUF_INDIRECT),
                       ("normal_depth", capi.BUF_NORMAL_DEPTH), ("combined", capi.BUF_COMBINED)):
        got = r.readback(kind)
        assert_same(got, ref[name], name)
    s = r.stats()
    assert (s.rays_primary, s.rays_extension, s.rays_shadow) == ref["rays"]
    r.close()


def fan_soup(seed, nquads, nsingles, fold):
    """Indexed quads triangulated as fans (a,b,c),(a,c,d) -- the form OBJ faces take -- plus loose triangles in between.  With
    fold > 0 the fourth vertex leaves the plane of the first three, so a ray can be inside both triangles of a pair."""
    rs = np.random.RandomState(seed)
    verts, idx = [], []
    order = ["q"] * nquads + ["s"] * nsingles
    rs.shuffle(order)
    for kind in order:
        c = rs.uniform(-1.5, 1.5, 3)
        u, v = rs.normal(size=3), rs.normal(size=3)
        u, v = 0.9 * u / np.linalg.norm(u), 0.9 * v / np.linalg.norm(v)
        base = len(verts)
        if kind == "q":
            n = np.cross(u, v)
            quad = [c, c + u, c + u + v + fold * n / max(np.linalg.norm(n), 1e-6) * rs.uniform(-1, 1), c + v]
            verts += quad
            idx += [base, base + 1, base + 2, base, base + 2, base + 3]
        else:
            verts += [c, c + u, c + v]
            idx += [base, base + 1, base + 2]
    pos = np.float32(verts)
    tri = pos[np.int64(idx)].reshape(-1, 3, 3)
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-12)
    nrm = np.zeros_like(pos)
    nrm[np.int64(idx)] = np.repeat(fn, 3, axis=0)  # last face wins at shared vertices: any finite normal will do
    uv = rs.rand(len(pos), 2).astype(np.float32)
    meshes = np.uint32([[len(pos), 0, len(idx), 0, 0, 0xFFFFFFFF, 0, 0]])
    return pos, nrm.astype(np.float32), uv, np.uint32(idx), meshes


@pytest.mark.parametrize("seed,nquads,nsingles,fold", [(21, 15, 0, 0.0), (22, 14, 5, 0.6), (23, 31, 2, 0.3), (24, 200, 77, 0.5)])
def test_fan_pairs_parity(native_lib, bluenoise, seed, nquads, nsingles, fold):
    """The exhaustive kernels test triangulated quads as fan pairs (shared tvec, q, edge product; one reciprocal unless a lane is
    inside both triangles).  Planar and folded quads, an odd number of pairs, loose triangles between them, more than 64
    triangles (forced exhaustive mode): exhaustive == LBVH == oracle brute force, bit for bit."""
    from oracle import cap_oracle as O
    pos, nrm, uv, idx, meshes = fan_soup(seed, nquads, nsingles, fold)
    w, h, D = 96, 80, 3
    r = capi.Renderer(0)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    cam = capi.CameraData()
    cam.position[:] = (0.2, 0.1, 6.0)
    cam.forward[:] = (0, 0, -1)
    cam.right[:] = (-1, 0, 0)
    cam.up[:] = (0, 1, 0)
    cam.focal_length = 0.03
    cam.sensor_size[0] = 0.036
    cam.sensor_size[1] = np.float32(0.036) * (np.float32(h) / np.float32(w))
    r.set_resolution(w, h)
    r.set_camera(cam)
    sc = O.Scene(pos, nrm, uv, idx, meshes)
    ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1], cam.focal_length)
    ref = sc.render_frame(ocam, bluenoise, w, h, 5, D, threads=8)
    assert ref["rays"][1] > 0.05 * w * h  # the camera sees the soup
    for mode in (2, 1):
        r.set_traversal(mode)
        r.stats_reset()
        r.render(5, 1, D, capi.RENDER_AOV)
        for name, kind in (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("direct", capi.BUF_DIRECT), ("indirect", capi.BUF_INDIRECT),
                           ("normal_depth", capi.BUF_NORMAL_DEPTH)):
            assert_same(r.readback(kind), ref[name], "%s (traversal %d)" % (name, mode))
        s = r.stats()
        assert (s.rays_primary, s.rays_extension, s.rays_shadow) == ref["rays"]
    r.close()


@pytest.mark.parametrize("build", [1, 2, 3, 4])
def test_geometric_progression_scene(native_lib, bluenoise, build):
    """Triangles whose size and distance grow geometrically: the SAH build wants to peel them off one by one (a tree as deep as
    the triangle count) and Morton codes collapse most of them into one cell.  Both builders must stay within the traversal
    stack and give the oracle's image."""
    from oracle import cap_oracle as O
    n = 120
    tris = []
    for k in range(n):
        s = 1.08 ** k
        x = 0.02 * s
        tris.append([[x, -0.01 * s, -0.002 * s], [x + 0.01 * s, 0.0, -0.002 * s], [x, 0.01 * s, -0.002 * s]])
    tris = np.float32(tris)
    pos = tris.reshape(-1, 3)
    nrm = np.tile(np.float32([0, 0, 1]), (len(pos), 1))
    uv = np.zeros((len(pos), 2), np.float32)
    idx = np.arange(len(pos), dtype=np.uint32)
    meshes = np.uint32([[len(pos), 0, len(pos), 0, 0, 0xFFFFFFFF, 0, 0]])
    r = capi.Renderer(0)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    r.upload_bluenoise(bluenoise)
    r.set_bvh_build(build)
    info = r.build_bvh()
    assert info.max_depth <= 64 and info.stack_entries >= min(info.max_depth, 32)
    nodes, leaves = r.bvh_readback()
    t3 = pos.reshape(-1, 3, 3)
    assert check_tree(nodes, leaves, t3.min(1), t3.max(1)) == info.max_depth
    w, h = 64, 48
    cam = capi.CameraData()
    cam.position[:] = (40.0, 0.0, 120.0)
    cam.forward[:] = (0, 0, -1)
    cam.right[:] = (-1, 0, 0)
    cam.up[:] = (0, 1, 0)
    cam.focal_length = 0.02
    cam.sensor_size[0] = 0.036
    cam.sensor_size[1] = np.float32(0.036) * (np.float32(h) / np.float32(w))
    r.set_resolution(w, h)
    r.set_camera(cam)
    r.set_traversal(1)
    r.render(1, 1, 2, capi.RENDER_AOV)
    sc = O.Scene(pos, nrm, uv, idx, meshes)
    ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1], cam.focal_length)
    ref = sc.render_frame(ocam, bluenoise, w, h, 1, 2, threads=4)
    assert (ref["gbuffer_geo"].view(np.uint32)[..., 3] != 0xFFFFFFFF).any()
    for name, kind in (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("indirect", capi.BUF_INDIRECT), ("direct", capi.BUF_DIRECT)):
        assert_same(r.readback(kind), ref[name], name)
    r.close()


def test_empty_scene_and_call_order(native_lib, bluenoise):
    r = capi.Renderer(0)
    with pytest.raises(capi.CapError):
        r.build_bvh()  # no scene
    r.upload_scene(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, np.uint32),
                   np.zeros((0, 8), np.uint32))
    r.upload_bluenoise(bluenoise)
    with pytest.raises(capi.CapError):
        r.render(0, 1, 1)  # BVH not built
    r.build_bvh()
    r.set_resolution(32, 16)
    r.set_camera(capi.cornell_camera(32, 16))
    r.render(0, 2, 3, capi.RENDER_AOV)
    c = r.readback(capi.BUF_COMBINED)
    assert np.all(c[..., :3] == np.float32([0.7, 0.7, 0.85]))  # every ray misses: sky
    with pytest.raises(capi.CapError):
        r.upload_scene(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), np.zeros((3, 2), np.float32), np.uint32([0, 1, 5]),
                       np.uint32([[3, 0, 3, 0, 0, 0xFFFFFFFF, 0, 0]]))  # index out of range is rejected on the host
    r.close()


@pytest.mark.parametrize("shape", [(16, 8), (5, 3), (1, 7), (7, 1), (2, 2)])
def test_textured_quad_parity(native_lib, bluenoise, shape):
    """Bilinear WRAP sampling from the footprint layout (cap_device.h TextureDev) against the oracle's four-texel form, on texture
    extents that are odd, one texel wide or one texel high (every neighbour wraps onto the texel itself), tiled twice across a quad."""
    from oracle import cap_oracle as O
    pos = np.float32([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [-3, -1, -1], [3, -1, -1], [3, 2, -1], [-3, 2, -1]])
    nrm = np.tile(np.float32([0, 0, 1]), (8, 1))
    uv = np.float32([[0, 0], [2, 0], [2, 2], [0, 2], [0.1, 0.2], [0.9, 0.2], [0.9, 0.7], [0.1, 0.7]])
    idx = np.uint32([0, 1, 2, 0, 2, 3, 0, 1, 2, 0, 2, 3])
    meshes = np.uint32([[4, 0, 6, 0, 0, 0, 0, 0], [4, 4, 6, 6, 1, 1, 0, 0]])
    rs = np.random.RandomState(5)
    tex0 = rs.randint(0, 256, shape + (4,)).astype(np.uint8)
    tex1 = np.zeros((4, 4, 4), np.uint8)  # black texture: kd == 0 terminates the path (rt_indirect.hlsl:108)
    tex1[::2, ::2] = 255
    w, h, D = 80, 60, 3
    r = capi.Renderer(0)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    r.upload_texture(0, tex0)
    r.upload_texture(1, tex1)
    r.upload_bluenoise(bluenoise)
    r.build_bvh()
    cam = capi.CameraData()
    cam.position[:] = (0.1, 0.3, 4.0)
    cam.forward[:] = (0, 0, -1)
    cam.right[:] = (-1, 0, 0)
    cam.up[:] = (0, 1, 0)
    cam.focal_length = 0.03
    cam.sensor_size[0] = 0.036
    cam.sensor_size[1] = np.float32(0.036) * (np.float32(h) / np.float32(w))
    r.set_resolution(w, h)
    r.set_camera(cam)
    r.render(9, 1, D, capi.RENDER_AOV)
    sc = O.Scene(pos, nrm, uv, idx, meshes, textures=[tex0, tex1])
    ocam = O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1], cam.focal_length)
    ref = sc.render_frame(ocam, bluenoise, w, h, 9, D)
    for name, kind in (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("albedo", capi.BUF_ALBEDO), ("direct", capi.BUF_DIRECT), ("indirect", capi.BUF_INDIRECT),
                       ("combined", capi.BUF_COMBINED)):
        got = r.readback(kind)
        assert_same(got, ref[name], name)
    # a missing texture is a 1x1 zero texel (texture_system.cpp:47-56): albedo 0 everywhere on that mesh
    r.upload_texture(0, None)
    r.render(9, 1, D, capi.RENDER_AOV)
    sc2 = O.Scene(pos, nrm, uv, idx, meshes, textures=[np.zeros((1, 1, 4), np.uint8), tex1])
    ref2 = sc2.render_frame(ocam, bluenoise, w, h, 9, D)
    assert np.array_equal(bits(r.readback(capi.BUF_COMBINED)), bits(ref2["combined"]))
    r.close()


@pytest.mark.parametrize("n,build", [(2, 1), (7, 1), (500, 1), (20000, 1), (20000, 2), (2, 3), (7, 3), (1500, 3), (20000, 3), (40, 4), (1500, 4), (20000, 4)])
def test_wide_view_structure_on_device(native_lib, n, build):
    """The compressed 8-wide view as cap_bvh_build leaves it on the device -- collapsed on the device itself for the device-built
    LBVH (bvh.hip k_wide_level), on the host for the SAH tree -- satisfies the structural and conservativeness checks of the host
    builder's CPU test (tests/test_host_wide.py walk): every triangle in exactly one leaf child, inner children contiguous in slot
    order, every decoded child box containing its triangles' padded boxes."""
    import test_host_wide as hw
    rs = np.random.RandomState(300 + n)
    tri = (rs.uniform(-4, 4, (n, 1, 3)) + rs.uniform(-0.3, 0.3, (n, 3, 3))).astype(np.float32)
    pos = tri.reshape(-1, 3)
    nrm = np.tile(np.float32([0, 1, 0]), (3 * n, 1))
    uv = np.zeros((3 * n, 2), np.float32)
    idx = np.arange(3 * n, dtype=np.uint32)
    meshes = np.uint32([[3 * n, 0, 3 * n, 0, 0, 0xFFFFFFFF, 0, 0]])
    r = capi.Renderer(0)
    r.set_bvh_build(build)
    r.upload_scene(pos, nrm, uv, idx, meshes)
    info = r.build_bvh()
    nodes, order = r.bvh_readback()
    wide, src, depth, top = r.bvh_wide_readback()
    lo, hi = tri.min(1), tri.max(1)
    d, _ = hw.walk(lo, hi, order, wide, src, np.float32(info.bounds_lo), np.float32(info.bounds_hi))
    assert d == depth and 1 <= top <= min(len(wide), 73)
    if n >= 20000:
        assert depth <= 14 and len(wide) < n // 3
    r.close()


@pytest.mark.parametrize("ntri", [33, 2000, 50000])
def test_sah_device_build_is_deterministic(native_lib, ntri):
    """CAP_BVH_BUILD_SAH_DEVICE (ploc.hip): bins are integer atomics, positions and node numbers come from prefix sums -- two builds of one
    scene give the same bytes, binary tree and 8-wide view alike (every rank of a multi-GPU job builds its own copy)."""
    pos, nrm, uv, idx, meshes = soup(40 + ntri % 7, ntri)
    out = []
    for _ in range(2):
        r = capi.Renderer(0)
        r.upload_scene(pos, nrm, uv, idx, meshes)
        r.set_bvh_build(capi.Renderer.BVH_BUILD_SAH_DEVICE)
        r.build_bvh()
        nodes, leaves = r.bvh_readback()
        wn, wsrc, _, _ = r.bvh_wide_readback()
        out.append((nodes.copy(), leaves.copy(), wn.copy(), wsrc.copy()))
        r.close()
    for a, b in zip(*out):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
