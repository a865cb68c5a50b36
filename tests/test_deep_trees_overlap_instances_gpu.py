"""cap_overlap_instances on small deep trees: deep_tree_support's spiral of n triangles under the host SAH builder is n - 2 levels deep,
so the sizes reach every traversal-stack class of k_overlap_inst (16 / 24 / 32 / 64 entries) from both sides.  The spiral is the
bottom-level tree of three instances about the origin -- the identity, a rotation and a mirrored anisotropic transform --, and
overlap_support.spiral_boxes is mapped through each of them: the image of a small box around the origin contains the object-space origin,
which every triangle's box contains, so its image box keeps both children at every level of that instance's walk, which enters child 0
and pushes child 1 and holds one stack entry per level before the first pop.  The model walker says so without a GPU -- it walks the host
builder's tree against the image box cap_debug_overlap_instance_prune reports --; the GPU's pages, instances and counts are held bit
for bit to the brute force of overlap_instances_support.py."""
import numpy as np
import pytest

from capsaicin_amd import capi
from deep_tree_support import SIZES, depth_of, mesh_masks, spiral, spiral_arrays, tri_boxes
from filter_support import mesh_of_triangles
from instance_support import rotation
from overlap_instances_support import PairTable, affine, assert_counts, assert_pair_pages, boxes_of, cursors_of, identity, pair_valid, prune
from overlap_support import box_walk, spiral_boxes
from refit_support import Scene, context
from test_deep_trees_overlap_gpu import stack_class, want_high_water

SAH = capi.Renderer.BVH_BUILD_SAH


def instances_of(n):
    rng = np.random.default_rng(n)
    R = rotation(rng)
    return np.stack([identity()[0], affine(R), affine(rotation(rng) @ np.diag([-1.0, 2.0, 0.5]) @ R.T)])


def mapped_boxes(n, M):
    """spiral_boxes(n) mapped through each instance: per box the world box of the images of its corners (the degenerate ones as they
    are, once)"""
    b = spiral_boxes(n)
    ok = np.isfinite(b[:, [0, 1, 2, 4, 5, 6]]).all(1) & (b[:, 0:3] <= b[:, 4:7]).all(1) & (np.abs(b[:, 0]) < 1e30)
    good = b[ok].astype(np.float64)
    corners = np.stack([np.where([(c >> k) & 1 for k in range(3)], good[:, 4:7], good[:, 0:3]) for c in range(8)], 1)
    out = []
    for m in np.asarray(M, np.float64):
        w = corners @ m[:, :3].T + m[:, 3]
        out.append(boxes_of(w.min(1).astype(np.float32), w.max(1).astype(np.float32)))
    return np.concatenate(out + [b[~ok]])


@pytest.mark.parametrize("n", SIZES)
def test_boxes_fill_the_stack(native_lib, n):
    """no GPU: the model walk of the host builder's tree against each instance's image box holds as many entries as the tree can ask
    for, and reaches every candidate of that instance"""
    tris, M = spiral(n), instances_of(n)
    nodes, order, depth = capi.host_sah_build(*tri_boxes(tris))
    assert depth == depth_of(n)
    boxes = mapped_boxes(n, M)
    tab = PairTable(boxes, M, tris)
    cnt = tab.counts()
    assert (cnt == 3 * n).sum() >= 10 and (cnt == 0).sum() >= 10 and ((cnt > 0) & (cnt < 3 * n)).sum() >= 40, "every pair, none, and some of them"
    olo, ohi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    for i, m in enumerate(M):
        high = 0
        for b in np.nonzero(~tab.bad)[0]:
            p = prune(m, olo, ohi, olo, ohi, olo, ohi, boxes[b, 0:3], boxes[b, 4:7])
            if not np.isfinite(p["image_lo"]).all() or not np.isfinite(p["image_hi"]).all():
                continue  # (the FLT_MAX box: its image opens everything)
            image = np.zeros(8, np.float32)
            image[0:3], image[4:7] = p["image_lo"], p["image_hi"]
            h, reached = box_walk(nodes, order, tris, image, 0.0)
            high = max(high, h)
            assert set(np.nonzero(tab.meets[b, i * n:(i + 1) * n])[0].tolist()) <= {g for g, _ in reached}, (i, b)
        assert want_high_water(n) <= high <= depth, "instance %d" % i


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_overlap_instances(native_lib, n):
    tris, M = spiral(n), instances_of(n)
    scene = Scene(*spiral_arrays(tris))
    masks, mot = mesh_masks(n), mesh_of_triangles(scene.meshes)
    tab = PairTable(mapped_boxes(n, M), M, tris)
    assert len(np.unique(tab.page(4)[1])) == 4, "every instance in the pages, and empty slots"
    r = context(scene, SAH)
    try:
        assert r.bvh_info().max_depth == depth_of(n), "the stack class under test is the one that runs"
        print("spiral n %d: depth %d, instanced box overlap walks take the %d-entry class" % (n, depth_of(n), stack_class(depth_of(n))))
        r.set_instances(M)
        for table, mask in ((False, None), (True, None), (True, 0x55), (True, 0x80)):
            if table:
                r.set_instance_masks(masks)
            t = tab.with_valid(None if not table else pair_valid(3, n, None, None, masks[mot], mask))
            what = "n %d mask %s" % (n, mask)
            want4 = t.page(4)
            tri, inst, got = r.overlap_instances(t.b, 4, counts=True, mask=mask)
            assert_pair_pages((tri, inst), want4[:2], what + ", k = 4 with counts")
            assert_counts(got, want4[2], what)
            tri, inst, got = r.overlap_instances(t.b, 4, counts=True, mask=mask, resume=(tri, inst))
            want_next = t.page(4, cursors_of(want4[0], want4[1]))
            assert_pair_pages((tri, inst), want_next[:2], what + ", k = 4 with counts, the next page")
            assert_counts(got, want_next[2], what + ", the next page")
            assert_pair_pages(r.overlap_instances(t.b, 16, mask=mask), t.page(16)[:2], what + ", k = 16")
            assert_pair_pages(r.overlap_instances(t.b, 1, mask=mask), t.page(1)[:2], what + ", k = 1")
    finally:
        r.close()
