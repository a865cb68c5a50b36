"""cap_signed_distance on small deep trees: deep_tree_support's spiral of n triangles under the host SAH builder is n - 2 levels deep,
so the sizes reach every traversal-stack class of k_closest_points<.., true> (16 / 24 / 32 / 64 entries) from both sides -- the signed
launcher picks its class by the same depth ladder as cap_closest_points', and test_signed_distance_gpu.py's meshes are all shallow.
Records bit for bit against the brute force of closest_point_support.py, the signed array bit for bit against the float32 sign
computation of signed_distance_support.py on the device's read-back table."""
import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import assert_records, bits, closest
from deep_tree_support import SIZES, depth_of, mesh_masks, point_set, spiral, spiral_arrays
from filter_support import mesh_of_triangles
from refit_support import Scene, context
from signed_distance_support import signed_of

pytestmark = pytest.mark.gpu
SAH = capi.Renderer.BVH_BUILD_SAH


def point_class(depth):
    return 16 if depth <= 16 else 24 if depth <= 24 else 32 if depth <= 32 else 64


@pytest.mark.parametrize("n", SIZES)
def test_signed_distance(native_lib, n):
    tris = spiral(n)
    scene = Scene(*spiral_arrays(tris))
    masks, mot = mesh_masks(n), mesh_of_triangles(scene.meshes)
    q = point_set(n)
    r = context(scene, SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n), "the stack class under test is the one that runs"
        print("spiral n %d: depth %d, signed-distance walks take the %d-entry class" % (n, depth_of(n), point_class(depth_of(n))))
        r.build_pseudonormals()
        table = r.pseudonormals()
        for with_table, mask in ((False, None), (True, None), (True, 0x55), (True, 0x80)):
            if with_table:
                r.set_instance_masks(masks)
            passes = None if mask is None else (masks[mot] & mask) != 0
            what = "n %d mask %s" % (n, mask)
            want = closest(q, tris, passes)[0]
            want_signed = signed_of(want, q, tris, table)
            rec, sgn = r.signed_distance(q, mask=mask)
            assert_records(rec, want, what)
            bad = np.nonzero(bits(sgn).reshape(-1) != bits(want_signed).reshape(-1))[0]
            assert len(bad) == 0, "%s: %d of %d signed distances differ, first %d: got %r want %r" % (
                what, len(bad), len(sgn), bad[0], float(sgn[bad[0]]), float(want_signed[bad[0]]))
    finally:
        r.close()
