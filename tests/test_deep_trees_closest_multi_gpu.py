"""cap_closest_points_multi on small deep trees: deep_tree_support's spiral of n triangles under the host SAH builder is n - 2 levels
deep, so the sizes reach every traversal-stack class of k_closest_points_multi (16 / 24 / 32 / 64 entries) from both sides.  Every
triangle's box contains the neighbourhood of the origin: a point near it keeps both children at every level, and with counts on the
bound never shrinks below the radius, so the walk holds one stack entry per level.  Pages and counts bit for bit against the brute force
of closest_multi_support.py."""
import numpy as np
import pytest

from capsaicin_amd import capi
from closest_multi_support import Table, assert_counts, assert_pages, cursors_of
from deep_tree_support import SIZES, depth_of, mesh_masks, point_set, spiral, spiral_arrays
from filter_support import mesh_of_triangles
from refit_support import Scene, context

pytestmark = pytest.mark.gpu
SAH = capi.Renderer.BVH_BUILD_SAH


def point_class(depth):
    return 16 if depth <= 16 else 24 if depth <= 24 else 32 if depth <= 32 else 64


@pytest.mark.parametrize("n", SIZES)
def test_closest_points_multi(native_lib, n):
    tris = spiral(n)
    scene = Scene(*spiral_arrays(tris))
    masks, mot = mesh_masks(n), mesh_of_triangles(scene.meshes)
    tab = Table(point_set(n), tris)
    cnt = tab.counts()
    assert (cnt == n).sum() >= 90 and (cnt == 0).sum() >= 10 and ((cnt > 0) & (cnt < n)).sum() >= 10, "whole chains, none, and parts of it"
    r = context(scene, SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n), "the stack class under test is the one that runs"
        print("spiral n %d: depth %d, multi closest-point walks take the %d-entry class" % (n, depth_of(n), point_class(depth_of(n))))
        for table, mask in ((False, None), (True, None), (True, 0x55), (True, 0x80)):
            if table:
                r.set_instance_masks(masks)
            t = tab.with_mask(None if mask is None else (masks[mot] & mask) != 0)
            what = "n %d mask %s" % (n, mask)
            want4, want_cnt = t.page(4)
            page, got = r.closest_points_multi(t.q, 4, counts=True, mask=mask)
            assert_pages(page, want4, what + ", k = 4 with counts")
            assert_counts(got, want_cnt, what)
            page, got = r.closest_points_multi(t.q, 4, counts=True, mask=mask, resume=page)
            want_next, cnt_next = t.page(4, cursors_of(want4))
            assert_pages(page, want_next, what + ", k = 4 with counts, the next page")
            assert_counts(got, cnt_next, what + ", the next page")
            assert_pages(r.closest_points_multi(t.q, 16, mask=mask), t.page(16)[0], what + ", k = 16")
    finally:
        r.close()
