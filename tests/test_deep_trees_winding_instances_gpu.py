"""cap_winding_instances on object trees deeper than each of its stack size classes: k_winding_inst is compiled once per class (16, 24,
32 and 64 entries, picked by the deepest tree below an instance) and drops a push beyond its stack silently, so a class too small for
its depth would lose whole subtrees -- the visit counts and the values would differ from the host walk and nothing would fault.  The
scenes are the spirals of tests/deep_tree_support.py under the host SAH builder, depth n - 2, shown by one sheared instance: both sides
of 16 | 17, 24 | 25 and 32 | 33, and one at 38."""
import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import bits, closest, queries
from deep_tree_support import SIZES, depth_of, point_set, scales, spiral, spiral_arrays
from refit_support import Scene, context
from winding_instances_support import State, affine, walk, walk32
from winding_support import root_code

pytestmark = pytest.mark.gpu

# (no translation: the spirals span many binades about the origin, and a translation would round their small end away in p' = W q)
SHEAR = affine(np.array([[1.0, 0.4, 0.0], [0.0, 1.25, -0.3], [0.0, 0.0, 0.75]]), (0.0, 0.0, 0.0))


def kept(n, pts, tris):
    """A point ON a triangle sees that triangle under +-2 pi by the sign of a rounding error (test_deep_trees_winding_gpu.py): the value
    is compared where the nearest triangle is at least 10^-3 of max(|p|, s_0) away in object space, the visit counts everywhere"""
    rec, _ = closest(queries(pts[:, 0:3]), tris)
    return np.sqrt(rec[:, 3].astype(np.float64)) >= 1e-3 * np.maximum(np.linalg.norm(pts[:, 0:3].astype(np.float64), axis=1), scales(n)[0])


@pytest.mark.parametrize("n", SIZES)
def test_winding_instances(native_lib, n):
    tris, obj_pts = spiral(n), point_set(n)
    keep = kept(n, obj_pts, tris)
    assert keep.mean() >= 0.7, "the random points are kept, the centroids are not"
    M = SHEAR[None]
    pts = queries((obj_pts[:, 0:3].astype(np.float64) @ M[0, :, 0:3].astype(np.float64).T + M[0, :, 3]).astype(np.float32))
    r = context(Scene(*spiral_arrays(tris)), capi.Renderer.BVH_BUILD_SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n)
        r.build_winding()
        r.set_instances(M)
        top, inst, _ = r.winding_instances_tables()
        info = r.winding_instances_info()
        nodes, order = r.bvh_readback()
        st = State(top, list(info.level_entries)[:info.levels], inst, r.instances_readback()[0], [root_code(n)], r.winding_table(), order, tris, M)
        for beta in (2.0, np.inf):
            want, want_visits = walk(st, pts, beta)
            w32, v32 = walk32(st, pts, beta)
            got, visits = r.winding_instances(pts, beta=beta, visits=True)
            assert np.array_equal(visits.astype(np.int64), v32) and np.array_equal(v32, want_visits), "n %d beta %s: visits" % (n, beta)
            if np.isinf(beta):
                assert (visits[:, 1] == 1).all() and (visits[:, 3] == n).all(), "every triangle, whatever the depth"
            # 8 x the host-measured |walk32 - walk| of the case, never below the visits' 2^-24 (test_winding_instances_gpu.py)
            measured = np.abs(w32 - want)[keep].max()
            tol = np.maximum(8.0 * measured, want_visits.sum(1) * 2.0 ** -24)
            err = np.abs(got.astype(np.float64) - want)
            print("spiral n %d beta %s: max |gpu - walk| %.3e over the kept points, host |walk32 - walk| %.3e (bound %.3e)" % (
                n, beta, err[keep].max(), measured, tol.min()))
            assert (err[keep] <= tol[keep]).all(), "n %d beta %s: worst %.3e" % (n, beta, err[keep].max())
            assert np.array_equal(bits(r.winding_instances(pts, beta=beta)), bits(got)), "two runs give the same bits"
    finally:
        r.close()
