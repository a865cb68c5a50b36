"""cap_sweep_spheres on trees whose depth crosses every traversal-stack size class (16 / 24 / 32 / 64): the spirals of
tests/deep_tree_support.py under the host SAH builder, with the sweeps of sweep_support.spiral_sweeps -- along and across the spiral's
axes --, which tests/test_sweep_spheres.py shows to fill the stack up to its last entry.  Bit for bit against the brute force, with
and without a mesh-mask table."""
import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import assert_records, bits
from deep_tree_support import SIZES, depth_of, mesh_masks, spiral, spiral_arrays
from filter_support import mesh_of_triangles
from refit_support import Scene, context
from sweep_support import MISS, spiral_sweeps, sweep_scene

pytestmark = pytest.mark.gpu


def stack_class(depth):
    return 16 if depth <= 16 else 24 if depth <= 24 else 32 if depth <= 32 else 64


@pytest.mark.parametrize("n", SIZES)
def test_sweep_spheres(native_lib, n):
    tris = spiral(n)
    scene = Scene(*spiral_arrays(tris))
    sweeps = spiral_sweeps(n)
    want, _ = sweep_scene(sweeps, tris)
    ids = bits(want)[:, 6]
    assert (ids == MISS).any() and (ids != MISS).sum() > len(ids) // 2
    masks, mot = mesh_masks(n), mesh_of_triangles(scene.meshes)
    r = context(scene, capi.Renderer.BVH_BUILD_SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n)
        print("spiral n %d: sweeps take the %d-entry class" % (n, stack_class(depth_of(n))))
        assert_records(r.sweep_spheres(sweeps), want, "n %d" % n)
        r.set_instance_masks(masks)
        assert_records(r.sweep_spheres(sweeps), want, "n %d, a table and every mask bit" % n)
        for mask in (0x01, 0x55):
            passes = (masks[mot] & mask) != 0
            assert_records(r.sweep_spheres(sweeps, mask=mask), sweep_scene(sweeps, tris, passes)[0], "n %d mask 0x%02x" % (n, mask))
    finally:
        r.close()
