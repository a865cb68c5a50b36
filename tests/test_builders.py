"""The restated tree builders of tests/builder_support.py, checked on the host before tests/test_builders_gpu.py trusts them: every
restated tree is a tree (check_tree of test_bvh_gpu.py), the sort is sorted() on (key, id), the clustering equals a naive
pure-Python version at tiny n and halves an all-ties array, the surface-area split takes the cheapest binned plane, and the cases of
the GPU file provably reach every path (bin counts 8 / 16 / 32, both kinds of median, cluster counts on both sides of 1024)."""
import math

import numpy as np
import pytest

import builder_support as B
from test_bvh_gpu import check_tree

F = np.float32
RESTATED = {"lbvh": B.lbvh, "ploc": B.ploc, "sah": lambda t: B.sah(t)[:3], "sah16": lambda t: B.sah(t, leaf=16)[:3]}


@pytest.mark.parametrize("name", sorted(RESTATED))
@pytest.mark.parametrize("n", [1, 2, 3, 33, 1000])
def test_restated_tree_is_a_tree(name, n):
    tris = B.soup_tris(n, n)
    nodes, leaves, depth = RESTATED[name](tris)
    assert nodes.shape == (max(n - 1, 0), 16)
    assert check_tree(nodes, leaves, tris.min(1), tris.max(1)) == depth


@pytest.mark.parametrize("name", sorted(RESTATED))
def test_traversal_links_fold_small_subtrees(name):
    """q3's traversal links: a subtree of at most CAP_LEAF_MAX triangles is the range code of its consecutive leaves"""
    tris = B.soup_tris(9, 200)
    nodes, leaves, _ = RESTATED[name](tris)
    link = np.ascontiguousarray(nodes[:, 12:16]).view(np.int32)
    for i in range(len(nodes)):
        for s in range(2):
            below = B.triangles_below(nodes, leaves, link[i, s])
            t = int(link[i, 2 + s])
            if len(below) <= B.LEAF_MAX:
                code = ~t & 0xFFFFFFFF
                first, cnt = code & ((1 << B.LEAF_SHIFT) - 1), (code >> B.LEAF_SHIFT) + 1
                assert t < 0 and sorted(int(x) for x in leaves[first:first + cnt]) == below
            else:
                assert t == link[i, s] >= 0


@pytest.mark.parametrize("pattern", B.KEY_PATTERNS)
def test_crafted_keys_reach_the_sort(pattern):
    """the crafted scenes produce exactly the keys asked for, and the sort restatement is sorted() on (key, id)"""
    n = 5000
    want = B.crafted_keys(pattern, n - 2)
    tris = B.crafted(pattern, n)
    lo, hi = B.tri_boxes(tris)
    codes = B.morton_codes(lo, hi)
    assert codes[0] == 0 and codes[1] == 0x3FFFFFFF and np.array_equal(codes[2:].astype(np.uint64), want)
    assert B.sort_order(codes).tolist() == [i for _, i in sorted((int(k), i) for i, k in enumerate(codes))]


def test_sort_is_sorted_with_equal_keys():
    tris = np.concatenate([B.soup_tris(3, 2000), B.grid_quads(1000)])  # the two triangles of a quad share a box
    codes = B.morton_codes(*B.tri_boxes(tris))
    assert len(set(codes.tolist())) < len(codes)  # some equal keys: the id decides
    assert B.sort_order(codes).tolist() == [i for _, i in sorted((int(k), i) for i, k in enumerate(codes))]


def test_morton_code_bit_order():
    """x bits highest: a step along x alone changes bit 2 of the cell triple, along z bit 0"""
    for axis, bit in ((0, 2), (1, 1), (2, 0)):
        cell = np.zeros(3, F)
        cell[axis] = 1
        tri = B.keyed_triangles([0])
        tri[2] += cell
        assert B.morton_codes(*B.tri_boxes(tri))[2] == 1 << bit


def naive_clustering(lo, hi, radius):
    """ploc.hip:7-11, as written there: nearest neighbour within `radius` positions by union surface area, mutual pairs merge into
    the lower position, the array is compacted in order, until one cluster is left.  Ties: closer positions first, then the pair
    whose lower position is even, then the lower position.  Pure Python, O(n^2 x iterations)."""
    n = len(lo)
    clusters = [(lo[i], hi[i], ~i) for i in range(n)]
    child = np.zeros((n - 1, 2), np.int64)
    next_node = n - 2
    while len(clusters) > 1:
        m = len(clusters)
        nn = []
        for i in range(m):
            best = None
            for j in range(m):
                if j == i or abs(j - i) > radius:
                    continue
                d = np.maximum(clusters[i][1], clusters[j][1]) - np.minimum(clusters[i][0], clusters[j][0])
                area = F(F(F(d[0] * d[1]) + F(d[1] * d[2])) + F(d[2] * d[0]))
                rank = (float(area), abs(j - i), min(i, j) & 1, min(i, j))
                if best is None or rank < best[0]:
                    best = (rank, j)
            nn.append(best[1])
        out = []
        for i in range(m):
            j = nn[i]
            if nn[j] == i and j < i:
                continue  # merged into the lower position
            if nn[j] == i:
                child[next_node] = (clusters[i][2], clusters[j][2])
                out.append((np.minimum(clusters[i][0], clusters[j][0]), np.maximum(clusters[i][1], clusters[j][1]), next_node))
                next_node -= 1
            else:
                out.append(clusters[i])
        clusters = out
    return child


@pytest.mark.parametrize("n,radius,kind", [(2, 16, "soup"), (3, 1, "soup"), (5, 2, "soup"), (8, 1, "grid"), (11, 3, "grid"), (12, 16, "soup"),
                                           (12, 2, "same"), (9, 1, "same"), (12, 1, "soup")])
def test_clustering_equals_the_naive_version(n, radius, kind):
    tris = {"soup": B.soup_tris, "grid": lambda s, n: B.grid_quads(n), "same": lambda s, n: B.identical(n)}[kind](n + radius, n)
    order, _, plo, phi = B.setup(tris)
    want = B.finish(n, naive_clustering(plo, phi, radius), order, plo, phi)
    B.assert_same_tree(B.ploc(tris, radius), want, "restated clustering against the naive version")


@pytest.mark.parametrize("n", [2, 3, 7, 64, 100, 1025, 3000])
@pytest.mark.parametrize("radius", [1, 16])
def test_all_ties_halve_the_array(n, radius):
    """identical triangles: every distance ties, the symmetric tie key pairs (0, 1), (2, 3), ... and the depth is ceil(log2 n)"""
    trace = []
    _, _, depth = B.ploc(B.identical(n), radius, trace)
    assert depth == math.ceil(math.log2(n))
    assert all(b == (a + 1) // 2 for a, b in zip(trace, trace[1:]))


# float32 cost of a plane = la * nl + ra * nr with la = dx * dy + dy * dz + dz * dx over float32 extents: a subtraction, a product and
# two sums per term of the area (all terms >= 0, so relative errors do not amplify): (1 + e)^4 per area, one more product by the
# exactly represented count and one sum: (1 + e)^6, e = 2^-24.  The chosen plane's exact cost is therefore within (1 + e)^6 / (1 - e)^6
# < 1 + 16 e of the exact minimum.
COST_SLACK = 1.0 + 16.0 * 2.0 ** -24


def exact_costs(seg):
    K = seg["K"]
    lo, hi, bins = seg["lo"].astype(np.float64), seg["hi"].astype(np.float64), seg["bins"]
    out = np.full((3, K - 1), np.inf)
    for ax in range(3):
        if not seg["ext_ok"][ax]:
            continue
        for b in range(K - 1):
            left = bins[:, ax] <= b
            if left.all() or not left.any():
                continue
            c = 0.0
            for side in (left, ~left):
                d = hi[side].max(0) - lo[side].min(0)
                c += (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]) * side.sum()
            out[ax, b] = c
    return out


@pytest.mark.parametrize("make,n,leaf", [(B.soup_tris, 200, 16), (B.soup_tris, 1500, 32), (lambda s, n: B.grid_quads(n), 300, 16)])
def test_sah_takes_the_cheapest_binned_plane(make, n, leaf):
    probe = []
    B.sah(make(n, n), leaf=leaf, probe=probe)
    assert len(probe) >= 4 and {seg["K"] for seg in probe} >= ({8, 16, 32} if n >= 1024 else {8, 16})
    ties = 0
    for seg in probe:
        exact = exact_costs(seg)
        assert np.array_equal(np.isfinite(exact), np.isfinite(seg["cost"]))  # the same candidate planes
        assert seg["decision"] is not None and seg["depth"] < B.SAH_MEDIAN_DEPTH
        ax, b, n_left, _ = seg["decision"]
        assert exact[ax, b] <= exact.min() * COST_SLACK
        assert n_left == (seg["bins"][:, ax] <= b).sum()
        # strict <: among equal float32 costs the first in (axis, bin) order
        same = np.argwhere(seg["cost"] == seg["cost"][ax, b])
        ties += len(same) > 1
        assert tuple(same[0]) == (ax, b)
    print("%d split segments, %d with tied float32 minima" % (len(probe), ties))


def test_sah_bin_counts_by_segment_size():
    assert B.sah_bins_for(np.array([33, 127, 128, 1023, 1024, 20000])).tolist() == [8, 8, 16, 16, 32, 32]


# ---- the cases of tests/test_builders_gpu.py reach every path ----
def test_gpu_cases_reach_every_sah_path():
    import deep_tree_support as D
    import test_builders_gpu as G
    total = {}
    for name, tris, leaf, radius in G.sah_cases():
        _, _, depth, paths = B.sah(tris, leaf=leaf, radius=radius)
        print("%-28s depth %d %s" % (name, depth, paths))
        assert depth <= 64  # what cap_bvh_build accepts
        for k, v in paths.items():
            total[k] = total.get(k, 0) + v
    assert total["K8"] > 0 and total["K16"] > 0 and total["K32"] > 0
    assert total["no_plane"] > 0 and total["depth_limit"] > 0
    # the two scenes that exist for the medians, by themselves
    deep = B.sah(D.spiral(G.SPIRAL_N), leaf=16)
    assert deep[3]["depth_limit"] == 3 and deep[3]["levels"] == 37 and deep[2] == 45 <= 64
    deep = B.sah(D.spiral(G.SPIRAL_N), leaf=32)
    assert deep[3]["depth_limit"] == 1 and deep[3]["levels"] == 36 and deep[2] == 53 <= 64
    same = B.sah(B.identical(3000))
    assert same[3]["no_plane"] == 127 and same[3]["K32"] == same[3]["K16"] == same[3]["K8"] == 0


def test_gpu_cases_cross_the_tail_threshold():
    """kPlocTail = 1024: a clustering case whose cluster count crosses it mid-build (main loop, then tail), cases that never exceed
    it (tail only), and one that starts exactly above it"""
    import test_builders_gpu as G
    seen = {}
    for name, tris, radius in G.ploc_cases():
        trace = []
        B.ploc(tris, radius, trace)
        above = sum(m > 1024 for m in trace)
        seen[name] = (above, len(trace) - above)
        print("%-28s iterations above 1024: %d, at or below: %d, counts %s" % (name, above, len(trace) - above, trace[:6]))
    assert any(a >= 2 and b >= 2 for a, b in seen.values())
    assert any(a == 0 for a, b in seen.values())
    assert any(a == 1 for a, b in seen.values())


# ---- the margin of the GPU quality test ----
# measured here: V(restated device SAH) / V(host SAH) - 1 on the two scenes of test_builders_gpu.test_tree_quality_against_the_host_sah
QUALITY_EXCESS = {"hall": -0.0049, "soup": -0.0359}


def test_quality_margin(native_lib):
    """The restated device SAH tree (= the device's, once the equality tests hold) against the host SAH tree, expected node visits:
    hall at scale 0.2 (10 838 triangles): 32.137 against 32.295, excess -0.49 %; soup of 12 000: 243.49 against 252.55, excess -3.59 %.
    The device tree is the better one on both, so m = max(0.01, 2 x excess) = 0.01 on both."""
    import refit_support as R
    import test_builders_gpu as G
    for name, tris in G.quality_scenes():
        sah, ploc, lbvh = (R.expected_node_visits(f(tris)[0]) for f in (B.sah, B.ploc, B.lbvh))
        host = G.host_sah_visits(tris)
        excess = sah / host - 1.0
        print("%s, %d triangles: V restated device SAH %.4f, clustering %.4f, LBVH %.4f, host SAH %.4f, excess %.5f" % (name, len(tris), sah, ploc, lbvh, host, excess))
        assert abs(excess - QUALITY_EXCESS[name]) < 5e-4
        assert G.QUALITY_MARGIN[name] == max(0.01, 2.0 * QUALITY_EXCESS[name])
        assert sah < ploc < lbvh
