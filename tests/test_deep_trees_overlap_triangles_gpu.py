"""cap_overlap_triangles on small deep trees: deep_tree_support's spiral of n triangles under the host SAH builder is n - 2 levels deep, so
the sizes reach every traversal-stack class of k_overlap_triangles (16 / 24 / 32 / 64 entries) from both sides.  Every triangle's box
contains the neighbourhood of the origin: a thin query triangle there keeps both children at every level, and the walk -- k_overlap_boxes'
own, against the box of the query's vertices -- enters child 0, the rest of the chain, and pushes child 1, the level's own triangle, so it
holds one stack entry per level before the first pop.  The model walker of overlap_support.py says so without a GPU; the GPU's pages and
counts are held bit for bit to the brute force."""
import numpy as np
import pytest

from capsaicin_amd import capi
from deep_tree_support import SIZES, depth_of, mesh_masks, spiral, spiral_arrays, tri_boxes
from filter_support import mesh_of_triangles
from overlap_support import box_walk, boxes_of
from overlap_triangles_support import TriTable, assert_counts, assert_pages, cursors_of, scene_slack, spiral_queries, vertices_of
from refit_support import Scene, context
from test_deep_trees_overlap_gpu import stack_class, want_high_water

SAH = capi.Renderer.BVH_BUILD_SAH


@pytest.mark.parametrize("n", SIZES)
def test_thin_triangles_fill_the_stack(native_lib, n):
    """no GPU: the model walk of the host builder's tree, against the box of each query's vertices, holds as many entries as the tree can
    ask for and reaches every candidate"""
    tris = spiral(n)
    nodes, order, depth = capi.host_sah_build(*tri_boxes(tris))
    assert depth == depth_of(n)
    tab = TriTable(spiral_queries(n), tris)
    cnt = tab.counts()
    assert (cnt == n).sum() >= 5 and (cnt == 0).sum() >= 10 and ((cnt > 0) & (cnt < n)).sum() >= 20, "whole chains, none, and parts of it"
    A = vertices_of(tab.b)
    boxes = boxes_of(A.min(1), A.max(1))
    slack = scene_slack(tris)
    walks = {i: box_walk(nodes, order, tris, boxes[i], slack) for i in np.nonzero(~tab.bad)[0]}
    high = max(h for h, _ in walks.values())
    assert want_high_water(n) <= high <= depth
    from_top = 0
    for i, (h, reached) in walks.items():
        assert set(np.nonzero(tab.meets[i])[0].tolist()) <= {g for g, _ in reached}, i
        from_top += any(slot == high - 1 and tab.meets[i, g] for g, slot in reached)
    assert from_top >= 5, "answers come out of the highest slot used"


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_overlap_triangles(native_lib, n):
    tris = spiral(n)
    scene = Scene(*spiral_arrays(tris))
    masks, mot = mesh_masks(n), mesh_of_triangles(scene.meshes)
    tab = TriTable(spiral_queries(n), tris)
    r = context(scene, SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n), "the stack class under test is the one that runs"
        print("spiral n %d: depth %d, triangle overlap walks take the %d-entry class" % (n, depth_of(n), stack_class(depth_of(n))))
        for table, mask in ((False, None), (True, None), (True, 0x55), (True, 0x80)):
            if table:
                r.set_instance_masks(masks)
            t = tab.with_mask(None if mask is None else (masks[mot] & mask) != 0)
            what = "n %d mask %s" % (n, mask)
            want4, want_cnt = t.page(4)
            page, got = r.overlap_triangles(t.b, 4, counts=True, mask=mask)
            assert_pages(page, want4, what + ", k = 4 with counts")
            assert_counts(got, want_cnt, what)
            page, got = r.overlap_triangles(t.b, 4, counts=True, mask=mask, resume=page)
            want_next, cnt_next = t.page(4, cursors_of(want4))
            assert_pages(page, want_next, what + ", k = 4 with counts, the next page")
            assert_counts(got, cnt_next, what + ", the next page")
            assert_pages(r.overlap_triangles(t.b, 16, mask=mask), t.page(16)[0], what + ", k = 16")
            assert_pages(r.overlap_triangles(t.b, 1, mask=mask), t.page(1)[0], what + ", k = 1")
    finally:
        r.close()
