"""The signed-distance references on the CPU (signed_distance_support.py): known answers of the float64 pseudonormal table, its
statistics, and the float32 sign of the query against the float64 winding number -- with the face-normal shortcut shown wrong on the
same points."""
import numpy as np
import pytest

from closest_point_support import bits
from signed_distance_support import (TRUTH_MESHES, box, face_normal_sign, mesh, pseudonormals, reference_table, signed_of, tetrahedron, truth_case)


def signed_volume(tris):
    t = np.asarray(tris, np.float64)
    return (t[:, 0] * np.cross(t[:, 1], t[:, 2])).sum() / 6.0


@pytest.mark.parametrize("name", TRUTH_MESHES + ("sphere soup",))
def test_meshes_are_closed_and_wound_outwards(name):
    tris = mesh(name)
    _, s = reference_table(name)
    assert s["degenerate_triangles"] == 0 and s["nonmanifold_edges"] == 0 and s["inconsistent_edges"] == 0 and signed_volume(tris) > 0
    if name.startswith("sphere"):
        # closest_point_support.sphere leaves its south pole open: sin(pi) is 1.2e-16, not 0, so every column has a pole vertex of its
        # own, 1e-16 apart.  Closed to the winding number and to every query; to the weld a mesh with two boundary edges per column.
        cols = 12 if name == "sphere" else 50
        assert s["closed"] == 0 and s["boundary_edges"] == 2 * cols
    else:
        assert s["closed"] == 1 and s["vertices"] - s["edges"] + len(tris) == (0 if name == "torus" else 2)
    assert len(tris) == {"tetrahedron": 4, "octahedron": 8, "box": 12, "torus": 256, "sphere": 264, "cone": 600, "sphere soup": 4900}[name]


@pytest.mark.parametrize("split", (0, 0b111111, 0b010110, 0b101001))
def test_box_corners_and_edges_whatever_the_tessellation(split):
    size = np.array([1.0, 2.0, 3.0])
    tris = box(tuple(size), split)
    table, s = pseudonormals(tris)
    assert (s["vertices"], s["edges"], s["closed"]) == (8, 18, 1)
    for g in range(12):
        for k in range(3):
            corner = tris[g, k].astype(np.float64)
            want = (np.pi / 2) * np.where(corner == 0, -1.0, 1.0)
            assert np.abs(table[g, 4 + k] - want).max() < 1e-14, (split, g, k)
            a, b = tris[g, k].astype(np.float64), tris[g, (k + 1) % 3].astype(np.float64)
            moving = a != b
            if moving.sum() == 1:  # an edge of the box: the sum of its two faces' normals
                mid = 0.5 * (a + b)
                want = np.where(moving, 0.0, np.where(mid == 0, -1.0, 1.0))
            else:  # a face's diagonal: that face twice
                want = 2 * table[g, 0]
            assert np.abs(table[g, 1 + k] - want).max() < 1e-14, (split, g, k)


def test_statistics():
    tet = tetrahedron()
    pick = lambda s, *keys: tuple(s[k] for k in keys)
    _, s = pseudonormals(tet)
    assert pick(s, "vertices", "edges", "boundary_edges", "nonmanifold_edges", "inconsistent_edges", "degenerate_triangles", "closed") == (4, 6, 0, 0, 0, 0, 1)
    _, s = pseudonormals(tet[:3])
    assert pick(s, "vertices", "edges", "boundary_edges", "closed") == (4, 6, 3, 0)
    flipped = tet.copy()
    flipped[3] = flipped[3][[0, 2, 1]]
    _, s = pseudonormals(flipped)
    assert pick(s, "boundary_edges", "nonmanifold_edges", "inconsistent_edges", "closed") == (0, 0, 3, 0)
    fins = np.float32([[(0, 0, 0), (0, 0, 1), (1, 0, 0)], [(0, 0, 0), (0, 0, 1), (0, 1, 0)], [(0, 0, 0), (0, 0, 1), (-1, -1, 0)]])
    _, s = pseudonormals(fins)
    assert pick(s, "vertices", "edges", "boundary_edges", "nonmanifold_edges", "closed") == (5, 7, 6, 1, 0)
    bad = np.concatenate([tet, np.float32([[(5, 5, 5), (5, 5, 5), (6, 5, 5)]]), np.float32([[(7, 7, 7), (8, 8, 8), (9, 9, 9)]]),
                          np.float32([[(np.nan, 0, 0), (1, 0, 0), (0, 1, 0)]])])
    table, s = pseudonormals(bad)
    assert pick(s, "vertices", "edges", "degenerate_triangles", "closed") == (4, 6, 3, 1)
    assert (bits(table[4:].astype(np.float32)) == 0).all(), "all seven entries of a degenerate triangle are +0"
    # -0 welds to +0
    neg = np.float32([[(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(-0.0, 0, -0.0), (0, 1, -0.0), (-1, 0, 0)]])
    _, s = pseudonormals(neg)
    assert pick(s, "vertices", "edges", "boundary_edges") == (4, 5, 4)


@pytest.mark.parametrize("name", TRUTH_MESHES)
def test_the_sign_against_the_winding_number(name):
    tris = mesh(name)
    q, rec, inside, keep = truth_case(name)
    assert len(keep) > 3900
    assert 50 <= inside.sum() <= len(keep) - 50, "points on both sides"
    table, _ = reference_table(name)
    signed = signed_of(rec, q, tris, table.astype(np.float32))[keep]
    assert np.isfinite(signed).all()
    wrong = int(((signed < 0) != inside).sum())
    wrong_face = int(((face_normal_sign(rec[keep], q[keep], tris) < 0) != inside).sum())
    print("%s: %d kept, %d inside, %d wrong signs, %d with the face normal" % (name, len(keep), inside.sum(), wrong, wrong_face))
    assert wrong == 0
    if name in ("tetrahedron", "octahedron", "cone"):
        assert wrong_face >= 1, "the scene discriminates: the returned triangle's own normal gets points wrong"
