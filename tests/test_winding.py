"""Winding numbers on the host: known answers of the float64 ground truth, the host restatement of cap_winding_numbers' walk
(winding_support.walk) against that brute force on a median-split tree, and the presence of the interface.  No GPU."""
import os
import re

import numpy as np
import pytest

from signed_distance_support import TRUTH_MESHES, mesh, winding_number
from winding_support import (BETAS, median_tree, moments, octant_triangle, open_cube, punctured, query_case, table32_of, unit_sphere, walk, walk32)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tree_of(tris, leaf=4):
    nodes, order = median_tree(tris, leaf)
    table, info = moments(nodes, order, tris)
    return nodes, order, table32_of(table), info


# ---- known answers ----
def test_octant_triangle_is_an_eighth_by_orientation():
    origin = np.zeros((1, 3))
    assert abs(winding_number(origin, octant_triangle())[0] - 0.125) < 1e-15
    assert abs(winding_number(origin, octant_triangle(flip=True))[0] + 0.125) < 1e-15


def test_open_cube_centre_is_five_sixths():
    assert abs(winding_number(np.full((1, 3), 0.5), open_cube())[0] - 5.0 / 6.0) < 1e-14


def test_duplicated_mesh_doubles_w():
    tris, pts, _, _ = query_case("torus")
    w = winding_number(pts, tris)
    assert np.abs(winding_number(pts, np.concatenate([tris, tris])) - 2.0 * w).max() < 1e-12


@pytest.mark.parametrize("name", TRUTH_MESHES)
def test_closed_meshes_give_zero_or_one(name):
    tris, pts, inside, _ = query_case(name)
    w = winding_number(pts, tris)
    assert np.abs(w - inside.astype(np.float64)).max() < 1e-6 and inside.any() and not inside.all()


# ---- the walk ----
@pytest.mark.parametrize("name", TRUTH_MESHES + ("open cube", "punctured sphere", "octant triangle"))
def test_walk_at_infinite_beta_is_the_brute_force(name):
    tris, pts, _, _ = query_case(name)
    if name == "punctured sphere":  # (4 892 triangles: a smaller one of the same kind keeps the host loop short)
        tris = punctured(mesh("sphere"), 8)[0]
    nodes, order, t32, _ = tree_of(tris)
    w, visits = walk(nodes, order, tris, t32, pts, np.inf)
    assert np.abs(w - winding_number(pts, tris)).max() <= 1e-12, name
    assert (visits[:, 0] == 0).all() and (visits[:, 1] == len(tris)).all(), "every triangle exactly once, no dipole"


@pytest.mark.parametrize("leaf", (1, 4, 8))
def test_walk_does_not_depend_on_the_leaf_size_at_infinite_beta(leaf):
    tris, pts, _, _ = query_case("torus")
    nodes, order, t32, _ = tree_of(tris, leaf)
    w, visits = walk(nodes, order, tris, t32, pts[:200], np.inf)
    assert np.abs(w - winding_number(pts[:200], tris)).max() <= 1e-12 and (visits[:, 1] == len(tris)).all()


@pytest.mark.parametrize("name", TRUTH_MESHES)
def test_no_kept_point_on_the_wrong_side_at_beta_two(name):
    tris, pts, inside, share = query_case(name)
    assert share >= 0.9, "the distance rule keeps at least 90 %% of the drawn points (%.3f)" % share
    nodes, order, t32, _ = tree_of(tris)
    w, visits = walk(nodes, order, tris, t32, pts, 2.0)
    wrong = np.nonzero((w >= 0.5) != inside)[0]
    print("%s: beta 2 max |w - truth| %.4f, mean visits far %.1f exact %.1f" % (name, np.abs(w - inside).max(), visits[:, 0].mean(), visits[:, 1].mean()))
    assert len(wrong) == 0, "%s: %d of %d kept points on the wrong side of 1/2, first %d: w %.4f" % (name, len(wrong), len(pts), wrong[0], w[wrong[0]])


def test_walk32_decides_as_walk_and_stays_close():
    """the float32 restatement makes the same far / near decisions (they are float32 in both) and its value differs by float32
    rounding only: the figure the GPU tolerance is made of (test_winding_gpu.MEASURED)"""
    tris, pts, _, _ = query_case("torus")
    nodes, order, t32, _ = tree_of(tris)
    for beta in BETAS:
        (w, v), (w32, v32) = walk(nodes, order, tris, t32, pts, beta), walk32(nodes, order, tris, t32, pts, beta)
        assert np.array_equal(v, v32)
        assert np.abs(w32 - w).max() < 1e-5


def test_moments_of_a_closed_mesh():
    tris = mesh("torus")
    nodes, order, t32, info = tree_of(tris)
    assert info["inner_nodes"] == len(tris) - 1 and info["degenerate_triangles"] == 0
    assert np.abs(info["root_n"]).max() < 1e-12 * info["total_area"], "the normals of a closed mesh sum to zero"
    # a ball about p~ of radius r covers the child's stored box
    boxes = nodes[:, 0:12].reshape(-1, 2, 2, 3).astype(np.float64)
    p, r = t32[:, :, 0:3].astype(np.float64), t32[:, :, 3].astype(np.float64)
    far = np.sqrt((np.maximum(np.abs(boxes[:, :, 0] - p), np.abs(boxes[:, :, 1] - p)) ** 2).sum(2))
    assert (r >= far).all() and (r <= far * (1 + 2.0 ** -21)).all()


def test_degenerate_triangles_contribute_nothing():
    tris = np.concatenate([mesh("octahedron"), np.float32([[(5, 5, 5), (5, 5, 5), (6, 5, 5)], [(7, 7, 7), (8, 8, 8), (9, 9, 9)]])])
    nodes, order, t32, info = tree_of(tris)
    assert info["degenerate_triangles"] == 2
    ref = moments(*median_tree(mesh("octahedron"))[0:2], mesh("octahedron"))[1]
    assert info["total_area"] == pytest.approx(ref["total_area"], rel=1e-15)


# ---- the interface ----
def test_header_and_renderer_have_the_winding_interface():
    from capsaicin_amd import capi
    header = open(os.path.join(ROOT, "include", "capsaicin_hip.h")).read()
    for fn in ("cap_winding_build", "cap_winding_drop", "cap_winding_readback", "cap_winding_numbers"):
        assert re.search(r"^int %s\(CapContext\* ctx" % fn, header, re.M), "%s is declared" % fn
        assert fn in capi.SYMBOLS
    for method in ("build_winding", "drop_winding", "winding_table", "winding_numbers"):
        assert callable(getattr(capi.Renderer, method, None)), "Renderer.%s" % method
