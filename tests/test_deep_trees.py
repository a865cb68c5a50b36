"""The inputs of tests/test_deep_trees_gpu.py, checked without a GPU: the host SAH builder makes of the spiral of n triangles a tree of
depth n - 2, and the model walkers of tests/deep_tree_support.py (the kernels' visiting order in float32) say that the query sets fill
the traversal stack up to the last entry such a tree can ask for and fetch answers out of that entry -- so that a walk compiled with
too small a stack for its depth would drop a push and answer wrongly."""
import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import closest
from deep_tree_support import SIZES, depth_of, point_set, point_walk, ray_set, ray_walk, spiral, tri_boxes
from multi_hit_support import MISS, all_hits
from test_host_sah import walk


def want_high_water(n):
    """depth - 1: the traversal pointers make one leaf range of the lowest inner node, so a walk descends depth - 1 nodes and pushes
    at most once in each.  n = 40: depth - 2 (the builder's median rule from level 36 on ends the chain differently)."""
    return depth_of(n) - (2 if n == 40 else 1)


@pytest.fixture(scope="module", params=SIZES)
def tree(request, native_lib):
    n = request.param
    tris = spiral(n)
    nodes, order, depth = capi.host_sah_build(*tri_boxes(tris))
    return n, tris, nodes, order, depth


def test_depth_is_n_minus_2(native_lib):
    """the builder's peel rule the GPU tests rely on: one outlier per level"""
    for n in range(16, 41):
        assert capi.host_sah_build(*tri_boxes(spiral(n)))[2] == n - 2, n


def test_tree_is_well_formed(tree):
    n, tris, nodes, order, depth = tree
    assert depth == depth_of(n)
    assert walk(nodes, order, *tri_boxes(tris)) == depth


def test_rays_fill_the_stack(tree):
    n, tris, nodes, order, depth = tree
    rays = ray_set(n)
    res = [ray_walk(nodes, order, tris, r) for r in rays if np.all(np.isfinite(r[[0, 1, 2, 4, 5, 6]])) and np.any(r[4:7] != 0) and r[7] > r[3]]
    high = max(h for h, _, _, _ in res)
    assert want_high_water(n) <= high <= depth
    assert any(g is not None and slot == high - 1 for _, g, slot, _ in res), "no answer comes out of the highest slot used"
    assert max(len(all_hits(r, tris)) for r in rays) > 16


def test_model_rays_agree_with_brute_force(tree):
    """the model is a walk of this tree: its winners are the brute force's"""
    n, tris, nodes, order, depth = tree
    for r in ray_set(n, with_degenerate=False)[::3]:
        hits = all_hits(r, tris)
        assert ray_walk(nodes, order, tris, r)[1] == (hits[0][3] if hits else None)


def test_points_fill_the_stack(tree):
    n, tris, nodes, order, depth = tree
    pts = point_set(n)
    want, table = closest(pts, tris)
    res = [point_walk(nodes, order, tris, q, table[i]) for i, q in enumerate(pts)]
    high = max(h for h, _, _, _ in res)
    assert want_high_water(n) <= high <= depth
    assert any(g is not None and slot == high - 1 for _, g, slot, _ in res), "no answer comes out of the highest slot used"
    ids = capi.closest_triangles(want)[0]
    assert [MISS if g is None else g for _, g, _, _ in res] == ids.tolist()
    assert (ids == MISS).any() and (ids != MISS).sum() > len(pts) // 2  # the radii exclude and include
