"""cap_signed_distance_instances on small deep trees: deep_tree_support's spiral of n triangles under the host SAH builder is n - 2
levels deep, so the sizes reach every traversal-stack class of k_closest_inst<.., true> (16 / 24 / 32 / 64 entries) from both sides.
The spiral is the bottom-level tree of three instances -- the identity, a rotation and a mirrored anisotropic transform, all about the
origin, whose neighbourhood every triangle's box contains.  The kernel's second phase, the flat walk of the winning instance's tree from
p' = W p with no radius, is what fills the deep stacks here: near the origin it keeps both children at every level.  Records, instances
and signed values bit for bit against the reference of signed_distance_instances_support.py on the device's read-back W and table (the
spiral is an open soup: the sign is defined, it does not mean inside)."""
import numpy as np
import pytest

from capsaicin_amd import capi
from closest_instances_support import affine, identity
from deep_tree_support import SIZES, depth_of, mesh_masks, point_set, spiral, spiral_arrays
from filter_support import mesh_of_triangles
from instance_support import rotation
from refit_support import Scene, context
from signed_distance_instances_support import assert_signed, pair_valid, signed_distance_instances

pytestmark = pytest.mark.gpu
SAH = capi.Renderer.BVH_BUILD_SAH


def point_class(depth):
    return 16 if depth <= 16 else 24 if depth <= 24 else 32 if depth <= 32 else 64


@pytest.mark.parametrize("n", SIZES)
def test_signed_distance_instances(native_lib, n):
    tris = spiral(n)
    scene = Scene(*spiral_arrays(tris))
    rng = np.random.default_rng(n)
    R = rotation(rng)
    M = np.stack([identity()[0], affine(R), affine(rotation(rng) @ np.diag([-1.0, 2.0, 0.5]) @ R.T)])
    masks, mot = mesh_masks(n), mesh_of_triangles(scene.meshes)
    q = point_set(n)
    r = context(scene, SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n), "the stack class under test is the one that runs"
        print("spiral n %d: depth %d, signed instanced walks take the %d-entry class" % (n, depth_of(n), point_class(depth_of(n))))
        r.build_pseudonormals()
        r.set_instances(M)
        W, table = r.instances_readback()[0], r.pseudonormals()
        for with_table, mask in ((False, None), (True, None), (True, 0x55), (True, 0x80)):
            if with_table:
                r.set_instance_masks(masks)
            valid = pair_valid(3, n, None, None, masks[mot] if with_table else None, mask)
            want = signed_distance_instances(q, M, W, tris, table, valid)
            if mask is None:
                hit = want[1] >= 0
                assert len(np.unique(want[1][hit])) == 3 and (~hit).sum() >= 10, "every instance answers, and some points miss"
                assert 10 <= (want[2][hit] < 0).sum() <= hit.sum() - 10, "both signs"
            assert_signed(r.signed_distance_instances(q, mask=mask), want, "n %d mask %s" % (n, mask))
    finally:
        r.close()
