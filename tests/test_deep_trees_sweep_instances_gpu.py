"""cap_sweep_instances on small deep trees: deep_tree_support's spiral of n triangles under the host SAH builder is n - 2 levels deep,
so the sizes reach every traversal-stack class of k_sweep_inst (16 / 24 / 32 / 64 entries) from both sides.  The spiral is the
bottom-level tree of three instances -- the identity, a rotation and a mirrored anisotropic transform, all about the origin -- and the
sweeps are sweep_support.spiral_sweeps, which tests/test_sweep_spheres.py shows to fill the stack up to its last entry, each mapped
through one of the three transforms (the identity's third is the scene form's walk; a rotated node's world box only grows).  Records
and instances bit for bit against the brute force of sweep_instances_support.py, with and without the mesh-mask table."""
import numpy as np
import pytest

from capsaicin_amd import capi
from deep_tree_support import SIZES, depth_of, mesh_masks, spiral, spiral_arrays
from filter_support import mesh_of_triangles
from instance_support import rotation
from refit_support import Scene, context
from sweep_instances_support import affine, assert_pairs, expected, identity, pair_valid
from sweep_support import spiral_sweeps

pytestmark = pytest.mark.gpu
SAH = capi.Renderer.BVH_BUILD_SAH


def stack_class(depth):
    return 16 if depth <= 16 else 24 if depth <= 24 else 32 if depth <= 32 else 64


def mapped(sweeps, M):
    """sweep k through transform k mod 3: origin and direction mapped, the radius and tmax kept (degenerate rows stay degenerate)"""
    q = np.array(sweeps, np.float32, copy=True)
    Md = np.asarray(M, np.float64)
    k = np.arange(len(q)) % len(Md)
    with np.errstate(all="ignore"):
        q[:, 0:3] = (np.einsum("nrk,nk->nr", Md[k][:, :, :3], q[:, 0:3].astype(np.float64)) + Md[k][:, :, 3]).astype(np.float32)
        q[:, 4:7] = np.einsum("nrk,nk->nr", Md[k][:, :, :3], q[:, 4:7].astype(np.float64)).astype(np.float32)
    return q


@pytest.mark.parametrize("n", SIZES)
def test_sweep_instances(native_lib, n):
    tris = spiral(n)
    scene = Scene(*spiral_arrays(tris))
    rng = np.random.default_rng(n)
    R = rotation(rng)
    M = np.stack([identity()[0], affine(R), affine(rotation(rng) @ np.diag([-1.0, 2.0, 0.5]) @ R.T)])
    masks, mot = mesh_masks(n), mesh_of_triangles(scene.meshes)
    q = mapped(spiral_sweeps(n), M)
    want = expected(q, M, tris)
    hit = want[1] >= 0
    assert len(np.unique(want[1][hit])) == 3 and (~hit).sum() >= 3 and hit.sum() > len(q) // 2, "every instance answers, and some sweeps miss"
    r = context(scene, SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n), "the stack class under test is the one that runs"
        print("spiral n %d: depth %d, instanced sweeps take the %d-entry class" % (n, depth_of(n), stack_class(depth_of(n))))
        r.set_instances(M)
        assert_pairs(r.sweep_instances(q), want, "n %d" % n)
        r.set_instance_masks(masks)
        for mask in (None, 0x55, 0x80):
            valid = pair_valid(3, n, None, None, masks[mot], mask)
            assert_pairs(r.sweep_instances(q, mask=mask), expected(q, M, tris, valid), "n %d mask %s" % (n, mask))
    finally:
        r.close()
