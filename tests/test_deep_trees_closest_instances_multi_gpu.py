"""cap_closest_instances_multi on small deep trees: deep_tree_support's spiral of n triangles under the host SAH builder is n - 2 levels
deep, so the sizes reach every traversal-stack class of k_closest_inst_multi (16 / 24 / 32 / 64 entries) from both sides.  The spiral is
the bottom-level tree of the three instances of test_deep_trees_closest_instances_gpu.py -- the identity, a rotation and a mirrored
anisotropic transform, all about the origin, whose neighbourhood every triangle's box contains: a point near it keeps both children at
every level of every instance, and with counts on the bound never shrinks below the radius, so the walk holds one stack entry per level.
Pages, instances and counts bit for bit against the brute force of closest_instances_multi_support.py."""
import numpy as np
import pytest

from capsaicin_amd import capi
from closest_instances_multi_support import PairTable, assert_counts, assert_pair_pages, cursors_of
from closest_instances_support import affine, identity, pair_valid
from deep_tree_support import SIZES, depth_of, mesh_masks, point_set, spiral, spiral_arrays
from filter_support import mesh_of_triangles
from instance_support import rotation
from refit_support import Scene, context

pytestmark = pytest.mark.gpu
SAH = capi.Renderer.BVH_BUILD_SAH


def point_class(depth):
    return 16 if depth <= 16 else 24 if depth <= 24 else 32 if depth <= 32 else 64


@pytest.mark.parametrize("n", SIZES)
def test_closest_instances_multi(native_lib, n):
    tris = spiral(n)
    scene = Scene(*spiral_arrays(tris))
    rng = np.random.default_rng(n)
    R = rotation(rng)
    M = np.stack([identity()[0], affine(R), affine(rotation(rng) @ np.diag([-1.0, 2.0, 0.5]) @ R.T)])
    masks, mot = mesh_masks(n), mesh_of_triangles(scene.meshes)
    tab = PairTable(point_set(n), M, tris)
    cnt = tab.counts()
    assert (cnt == 3 * n).sum() >= 10 and (cnt == 0).sum() >= 10 and ((cnt > 0) & (cnt < 3 * n)).sum() >= 10, "every pair, none, and some of them"
    assert len(np.unique(tab.page(4)[1])) == 4, "every instance in the pages, and misses"
    r = context(scene, SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n), "the stack class under test is the one that runs"
        print("spiral n %d: depth %d, instanced multi closest-point walks take the %d-entry class" % (n, depth_of(n), point_class(depth_of(n))))
        r.set_instances(M)
        for table, mask in ((False, None), (True, None), (True, 0x55), (True, 0x80)):
            if table:
                r.set_instance_masks(masks)
            t = tab.with_valid(None if not table else pair_valid(3, n, None, None, masks[mot], mask))
            what = "n %d mask %s" % (n, mask)
            want4 = t.page(4)
            rec, inst, got = r.closest_instances_multi(t.q, 4, counts=True, mask=mask)
            assert_pair_pages((rec, inst), want4[:2], what + ", k = 4 with counts")
            assert_counts(got, want4[2], what)
            rec, inst, got = r.closest_instances_multi(t.q, 4, counts=True, mask=mask, resume=(rec, inst))
            want_next = t.page(4, cursors_of(want4[0], want4[1]))
            assert_pair_pages((rec, inst), want_next[:2], what + ", k = 4 with counts, the next page")
            assert_counts(got, want_next[2], what + ", the next page")
            assert_pair_pages(r.closest_instances_multi(t.q, 4, mask=mask), want4[:2], what + ", k = 4")
            assert_pair_pages(r.closest_instances_multi(t.q, 16, mask=mask), t.page(16)[:2], what + ", k = 16")
    finally:
        r.close()
