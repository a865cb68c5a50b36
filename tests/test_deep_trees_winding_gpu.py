"""cap_winding_numbers on trees deeper than each of its stack size classes: k_winding is compiled once per class (16, 24, 32 and 64
entries, picked by the tree's depth) and drops a push beyond its stack silently, so a class too small for its depth would lose whole
subtrees -- the visit counts and the values would differ from the host walk and nothing would fault.  The scenes are the spirals of
tests/deep_tree_support.py under the host SAH builder, depth n - 2: both sides of 16 | 17, 24 | 25 and 32 | 33, and one at 38."""
import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import bits, closest, queries
from deep_tree_support import SIZES, depth_of, point_set, scales, spiral, spiral_arrays
from refit_support import Scene, context
from winding_support import moments, walk

pytestmark = pytest.mark.gpu

# max |walk32 - walk| over the kept points of each spiral at beta = 2 and inf, measured on the host on winding_support.median_tree
# (leaf 4); the device's bound is 8 x this and never below (visits[0] + visits[1]) 2^-24 (test_winding_gpu.py has the reasons)
MEASURED = {18: 4.964e-07, 19: 5.042e-07, 26: 4.759e-07, 27: 5.254e-07, 34: 6.567e-07, 35: 5.963e-07, 40: 6.756e-07}


def kept(n, pts, tris):
    """A point ON a triangle -- point_set(n) holds every centroid -- sees that triangle under +-2 pi by the sign of a rounding error:
    the value is compared where the nearest triangle is at least 10^-3 of max(|p|, s_0) away, the visit counts everywhere"""
    rec, _ = closest(queries(pts[:, 0:3]), tris)
    return np.sqrt(rec[:, 3].astype(np.float64)) >= 1e-3 * np.maximum(np.linalg.norm(pts[:, 0:3].astype(np.float64), axis=1), scales(n)[0])


@pytest.mark.parametrize("n", SIZES)
def test_winding_numbers(native_lib, n):
    tris, pts = spiral(n), point_set(n)
    keep = kept(n, pts, tris)
    assert keep.mean() >= 0.7, "the random points are kept, the centroids are not"
    r = context(Scene(*spiral_arrays(tris)), capi.Renderer.BVH_BUILD_SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n)
        info = r.build_winding()
        nodes, order = r.bvh_readback()
        table = r.winding_table()
        assert info.inner_nodes == n - 1 and info.degenerate_triangles == moments(nodes, order, tris)[1]["degenerate_triangles"] == 0
        for beta in (2.0, np.inf):
            want, want_visits = walk(nodes, order, tris, table, pts, beta)
            got, visits = r.winding_numbers(pts, beta=beta, visits=True)
            assert np.array_equal(visits.astype(np.int64), want_visits), "n %d beta %s: visits" % (n, beta)
            if np.isinf(beta):
                assert (visits[:, 0] == 0).all() and (visits[:, 1] == n).all(), "every triangle, whatever the depth"
            tol = np.maximum(8.0 * MEASURED[n], want_visits.sum(1) * 2.0 ** -24)
            err = np.abs(got.astype(np.float64) - want)
            print("spiral n %d beta %s: max |gpu - walk| %.3e over the kept points (bound %.3e)" % (n, beta, err[keep].max(), tol.min()))
            assert (err[keep] <= tol[keep]).all(), "n %d beta %s: worst %.3e" % (n, beta, err[keep].max())
            assert np.array_equal(bits(r.winding_numbers(pts, beta=beta)), bits(got)), "two runs give the same bits"
    finally:
        r.close()
