"""cap_closest_instances on small deep trees: deep_tree_support's spiral of n triangles under the host SAH builder is n - 2 levels deep,
so the sizes reach every traversal-stack class of k_closest_inst (16 / 24 / 32 / 64 entries) from both sides.  The spiral is the
bottom-level tree of three instances -- the identity, a rotation and a mirrored anisotropic transform, all about the origin, whose
neighbourhood every triangle's box contains: a point near it keeps both children at every level of every instance.  Records and
instances bit for bit against the brute force of closest_instances_support.py."""
import numpy as np
import pytest

from capsaicin_amd import capi
from closest_instances_support import affine, assert_pairs, closest_instances, identity, pair_valid
from deep_tree_support import SIZES, depth_of, mesh_masks, point_set, spiral, spiral_arrays
from filter_support import mesh_of_triangles
from instance_support import rotation
from refit_support import Scene, context

pytestmark = pytest.mark.gpu
SAH = capi.Renderer.BVH_BUILD_SAH


def point_class(depth):
    return 16 if depth <= 16 else 24 if depth <= 24 else 32 if depth <= 32 else 64


@pytest.mark.parametrize("n", SIZES)
def test_closest_instances(native_lib, n):
    tris = spiral(n)
    scene = Scene(*spiral_arrays(tris))
    rng = np.random.default_rng(n)
    R = rotation(rng)
    M = np.stack([identity()[0], affine(R), affine(rotation(rng) @ np.diag([-1.0, 2.0, 0.5]) @ R.T)])
    masks, mot = mesh_masks(n), mesh_of_triangles(scene.meshes)
    q = point_set(n)
    want = closest_instances(q, M, tris)
    assert len(np.unique(want[1][want[1] >= 0])) == 3 and (want[1] < 0).sum() >= 10, "every instance answers, and some points miss"
    r = context(scene, SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n), "the stack class under test is the one that runs"
        print("spiral n %d: depth %d, instanced closest-point walks take the %d-entry class" % (n, depth_of(n), point_class(depth_of(n))))
        r.set_instances(M)
        assert_pairs(r.closest_instances(q), want, "n %d" % n)
        r.set_instance_masks(masks)
        for mask in (None, 0x55, 0x80):
            valid = pair_valid(3, n, None, None, masks[mot], mask)
            assert_pairs(r.closest_instances(q, mask=mask), closest_instances(q, M, tris, valid), "n %d mask %s" % (n, mask))
    finally:
        r.close()
