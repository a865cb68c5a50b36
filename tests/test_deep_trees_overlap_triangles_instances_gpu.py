"""cap_overlap_triangles_instances on small deep trees: deep_tree_support's spiral of n triangles under the host SAH builder is n - 2
levels deep, so the sizes reach every traversal-stack class of k_overlap_tri_inst (16 / 24 / 32 / 64 entries) from both sides.  The spiral
is the bottom-level tree of three instances about the origin -- the identity, a rotation and a mirrored anisotropic transform --, and
overlap_triangles_support.spiral_queries is mapped through each of them: the image of a thin triangle from the origin lies about the world
origin, which the world box of every node box contains, so the walk keeps both children at every level of that instance, enters child 0,
pushes child 1 and holds one stack entry per level before the first pop.  The model walker says so without a GPU -- it walks the host
builder's tree with the numpy model of world_node_step --; the GPU's pages, instances and counts are held bit for bit to the brute force
of overlap_triangles_instances_support.py."""
import numpy as np
import pytest

from capsaicin_amd import capi
from deep_tree_support import SIZES, depth_of, mesh_masks, spiral, spiral_arrays, tri_boxes
from filter_support import mesh_of_triangles
from overlap_triangles_instances_support import (TriPairTable, assert_counts, assert_pair_pages, cursors_of, pair_valid, queries_of_tris, query_boxes,
                                                 vertices_of, world_node, world_walk)
from overlap_triangles_support import spiral_queries
from refit_support import Scene, context
from test_deep_trees_overlap_gpu import stack_class, want_high_water
from test_deep_trees_overlap_instances_gpu import instances_of

SAH = capi.Renderer.BVH_BUILD_SAH


def mapped_queries(n, M):
    """spiral_queries(n) mapped through each instance, vertex by vertex (the queries that are not traversed as they are, once)"""
    q = spiral_queries(n)
    A = vertices_of(q)
    ok = np.isfinite(A).all((1, 2))
    good = A[ok].astype(np.float64)
    out = [queries_of_tris((good @ m[:, :3].T + m[:, 3]).astype(np.float32)) for m in np.asarray(M, np.float64)]
    return np.concatenate(out + [q[~ok]])


@pytest.mark.parametrize("n", SIZES)
def test_thin_triangles_fill_the_stack(native_lib, n):
    """no GPU: the model walk of the host builder's tree under each instance holds as many entries as the tree can ask for, and reaches
    every candidate of that instance"""
    tris, M = spiral(n), instances_of(n)
    nodes, order, depth = capi.host_sah_build(*tri_boxes(tris))
    assert depth == depth_of(n)
    q = mapped_queries(n, M)
    tab = TriPairTable(q, M, tris)
    cnt = tab.counts()
    assert (cnt >= n).sum() >= 5 and (cnt == 0).sum() >= 10 and ((cnt > 0) & (cnt < n)).sum() >= 20, "whole chains, none, and parts of it"
    olo, ohi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    qlo, qhi = query_boxes(q)
    for i, m in enumerate(M):
        xw = world_node(m, olo, ohi, olo, ohi, qlo[0], qhi[0])["xw"]
        high = 0
        for b in np.nonzero(~tab.bad & tab.meets[:, i * n:(i + 1) * n].any(1))[0]:
            h, reached = world_walk(nodes, order, m, xw, qlo[b], qhi[b])
            high = max(high, h)
            assert set(np.nonzero(tab.meets[b, i * n:(i + 1) * n])[0].tolist()) <= set(reached), (i, b)
        assert want_high_water(n) <= high <= depth, "instance %d" % i


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_overlap_triangles_instances(native_lib, n):
    tris, M = spiral(n), instances_of(n)
    scene = Scene(*spiral_arrays(tris))
    masks, mot = mesh_masks(n), mesh_of_triangles(scene.meshes)
    tab = TriPairTable(mapped_queries(n, M), M, tris)
    assert len(np.unique(tab.page(4)[1])) == 4, "every instance in the pages, and empty slots"
    r = context(scene, SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n), "the stack class under test is the one that runs"
        print("spiral n %d: depth %d, instanced triangle overlap walks take the %d-entry class" % (n, depth_of(n), stack_class(depth_of(n))))
        r.set_instances(M)
        for table, mask in ((False, None), (True, None), (True, 0x55), (True, 0x80)):
            if table:
                r.set_instance_masks(masks)
            t = tab.with_valid(None if not table else pair_valid(3, n, None, None, masks[mot], mask))
            what = "n %d mask %s" % (n, mask)
            want4 = t.page(4)
            tri, inst, got = r.overlap_triangles_instances(t.b, 4, counts=True, mask=mask)
            assert_pair_pages((tri, inst), want4[:2], what + ", k = 4 with counts")
            assert_counts(got, want4[2], what)
            tri, inst, got = r.overlap_triangles_instances(t.b, 4, counts=True, mask=mask, resume=(tri, inst))
            want_next = t.page(4, cursors_of(want4[0], want4[1]))
            assert_pair_pages((tri, inst), want_next[:2], what + ", k = 4 with counts, the next page")
            assert_counts(got, want_next[2], what + ", the next page")
            assert_pair_pages(r.overlap_triangles_instances(t.b, 16, mask=mask), t.page(16)[:2], what + ", k = 16")
            assert_pair_pages(r.overlap_triangles_instances(t.b, 1, mask=mask), t.page(1)[:2], what + ", k = 1")
    finally:
        r.close()
