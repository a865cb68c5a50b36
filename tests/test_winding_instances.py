"""Winding numbers over instances on the host: known answers of the world definition, the host restatement of cap_winding_instances'
two-level walk (winding_instances_support.walk) against the float64 brute force over the flattened scene, on tables built on the host,
and the presence of the interface.  No GPU."""
import os
import re

import numpy as np
import pytest

from signed_distance_support import box, mesh, winding_number
from winding_instances_support import (IDENTITY, affine, brute_force, grid_transforms, host_state, points_about, rotation, walk, walk32)
from winding_support import octant_triangle, open_cube

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIRROR = affine(np.diag([1.0, 1.0, -1.0]), (0, 0, 3))  # z -> 3 - z


def at(*xyz):
    return np.float32([list(xyz) + [np.inf]])


# ---- known answers ----
def test_a_mirrored_closed_box_reads_one_inside():
    tris = box((1.0, 2.0, 3.0))
    st, on = host_state(tris, MIRROR[None])
    q = np.concatenate([at(0.5, 1.0, 1.5), at(0.5, 1.0, 4.0)])
    assert np.abs(brute_force(q, MIRROR[None], on, tris) - [1.0, 0.0]).max() < 1e-14
    for beta in (2.0, np.inf):
        assert np.abs(walk(st, q, beta)[0] - [1.0, 0.0]).max() < 0.05, "the walk, and not -1: s_i is in the terms"
    assert np.abs(winding_number(q, tris @ np.diag([1.0, 1.0, -1.0]) + [0, 0, 3]) - [-1.0, 0.0]).max() < 1e-14, "without s_i a mirror turns the mesh inside out"


def test_two_overlapping_instances_read_two_in_the_overlap():
    tris = box((1.0, 1.0, 1.0))
    M = np.stack([IDENTITY, affine(np.eye(3), (0.5, 0, 0))])
    st, on = host_state(tris, M)
    q = np.concatenate([at(0.75, 0.5, 0.5), at(0.25, 0.5, 0.5), at(1.25, 0.5, 0.5), at(2.0, 0.5, 0.5)])
    want = [2.0, 1.0, 1.0, 0.0]
    assert np.abs(brute_force(q, M, on, tris) - want).max() < 1e-14
    for beta in (2.0, np.inf):
        assert np.abs(walk(st, q, beta)[0] - want).max() < 0.05


def test_an_open_cube_under_a_nonuniform_scale_is_measured_in_world_space():
    """solid angle is not affine-invariant: at the centre of the cube stretched to height 3 the missing top face subtends less than a
    sixth of the sphere, so w is the brute force on the SCALED cube and not the 5/6 of the pulled-back point"""
    tris = open_cube()
    M = affine(np.diag([1.0, 1.0, 3.0]), (0, 0, 0))[None]
    st, on = host_state(tris, M)
    q = at(0.5, 0.5, 1.5)
    scaled = (tris.astype(np.float64) * [1.0, 1.0, 3.0])
    truth = winding_number(q, scaled)[0]
    assert abs(brute_force(q, M, on, tris)[0] - truth) < 1e-15
    assert abs(walk(st, q, np.inf)[0][0] - truth) <= 1e-12
    assert abs(truth - 5.0 / 6.0) > 0.05 and truth > 5.0 / 6.0, truth


def test_a_mask_of_zero_switches_an_instance_off():
    tris = box((1.0, 1.0, 1.0))
    M = np.stack([IDENTITY, affine(np.eye(3), (0.5, 0, 0)), affine(np.eye(3), (4.0, 0, 0))])
    st, on = host_state(tris, M, masks=[0xFF, 0x00, 0x01])
    assert on.tolist() == [True, False, True]
    w, visits = walk(st, np.concatenate([at(0.75, 0.5, 0.5), at(4.5, 0.5, 0.5)]), np.inf)
    assert np.abs(w - [1.0, 1.0]).max() <= 1e-12 and (visits[:, 1] == 2).all() and (visits[:, 3] == 24).all()
    st, on = host_state(tris, M, masks=[0, 0, 0])
    w, visits = walk(st, at(0.75, 0.5, 0.5), 2.0)
    assert w[0] == 0.0 and not visits.any(), "no contributing instance: 0.0"


# ---- the walk ----
def cases():
    rng = np.random.default_rng(21)
    shear = np.array([[1.0, 0.4, 0.0], [0.0, 1.25, -0.3], [0.0, 0.0, 0.75]])
    mixed = np.stack([IDENTITY, affine(rotation(rng) @ np.diag([0.5, 1.0, 1.5]), (3, 0, 0)), affine(shear, (0, 3, 0)),
                      affine(rotation(rng) @ np.diag([1.0, 1.0, -1.0]), (0, 0, 3)), affine(2.0 * np.eye(3), (4096, 0, 0))])
    parts = [mesh("tetrahedron"), mesh("torus") + np.float32([8, 0, 0]), octant_triangle() + np.float32([0, 8, 0])]
    ranges = [(0, len(parts[0])), (len(parts[0]), len(parts[1])), (len(parts[0]) + len(parts[1]), 1)]
    return {
        "identity": (open_cube(), IDENTITY[None], None, None),
        "two": (open_cube(), mixed[:2], None, None),
        "three": (mesh("tetrahedron"), mixed[:3], None, None),
        "five": (open_cube(), mixed, None, None),
        "grid": (open_cube(), grid_transforms(2), None, None),
        "objects": (np.concatenate(parts).astype(np.float32), np.concatenate([mixed[:4], mixed[1:3]]), ranges, np.array([0, 1, 2, 1, 2, 0])),
    }


@pytest.mark.parametrize("name", tuple(cases()))
def test_walk_at_infinite_beta_is_the_brute_force(name):
    tris, M, ranges, objects = cases()[name]
    st, on = host_state(tris, M, ranges=ranges, objects=objects)
    q = points_about(np.random.default_rng(5), M[:4], on[:4], tris, 200, ranges=ranges, objects=objects)
    w, visits = walk(st, q, np.inf)
    truth = brute_force(q, M, on, tris, ranges, objects)
    assert np.abs(w - truth).max() <= 1e-12, name
    per = [len(tris) if ranges is None else ranges[objects[i]][1] for i in range(len(M))]
    assert (visits[:, 0] == 0).all() and (visits[:, 2] == 0).all() and (visits[:, 1] == len(M)).all() and (visits[:, 3] == sum(per)).all()


@pytest.mark.parametrize("n", (2, 4))
def test_no_kept_point_on_the_wrong_side_at_beta_two(n):
    """n^3 open cubes on a grid of pitch 3, each under rotation x diag(0.5 .. 1.5), every third mirrored.  Kept: |truth - 1/2| >= 0.1, the
    scene tests' cap on the error at beta = 2 twice over (include/capsaicin_hip.h: near 0.05)"""
    tris, M = open_cube(), grid_transforms(n)
    st, on = host_state(tris, M)
    q = points_about(np.random.default_rng(6), M, on, tris, 1500)
    truth = brute_force(q, M, on, tris)
    keep = np.abs(truth - 0.5) >= 0.1
    assert keep.mean() >= 0.9
    for beta, cap in ((2.0, 0.05), (4.0, 0.02)):
        w, visits = walk(st, q, beta)
        err = np.abs(w - truth)
        print("%d cubes beta %s: max |w - truth| %.4f, mean visits %s" % (n ** 3, beta, err.max(), visits.mean(0).round(1).tolist()))
        assert np.array_equal(w[keep] >= 0.5, truth[keep] >= 0.5), "a kept point on the wrong side of 1/2"
        assert err.max() < cap
    if n == 4:
        assert walk(st, q, 2.0)[1][:, 0].mean() > 1.0, "the top level takes far terms"


@pytest.mark.parametrize("name", ("five", "grid", "objects"))
def test_walk32_decides_as_walk_and_stays_close(name):
    tris, M, ranges, objects = cases()[name]
    st, on = host_state(tris, M, ranges=ranges, objects=objects)
    q = points_about(np.random.default_rng(7), M[:4], on[:4], tris, 300, ranges=ranges, objects=objects)
    for beta in (2.0, 4.0, np.inf):
        (w, v), (w32, v32) = walk(st, q, beta), walk32(st, q, beta)
        assert np.array_equal(v, v32)
        print("%s beta %s: max |walk32 - walk| %.3e" % (name, beta, np.abs(w32 - w).max()))
        assert np.abs(w32 - w).max() < 1e-4


def test_the_identity_instance_walks_as_the_scene():
    """sigma = 1 and |det L| = 1 exactly: below the instance every decision is the scene walk's"""
    from winding_support import walk as scene_walk
    tris = mesh("torus")
    st, on = host_state(tris, IDENTITY[None])
    assert st.inst[0, 9] == 1.0 and st.inst[0, 10] == 1.0 and st.inst[0, 11] == 1.0
    q = points_about(np.random.default_rng(8), IDENTITY[None], on, tris, 300)
    w, v = walk32(st, q, 2.0)
    from winding_support import median_tree, walk32 as scene_walk32
    nodes, order = median_tree(tris)
    ws, vs = scene_walk32(nodes, order, tris, st.table32, q, 2.0)
    near = v[:, 0] == 0
    assert near.any() and np.array_equal(v[near][:, 2:4], vs[near]) and np.array_equal(w[near], ws[near])
    del scene_walk


# ---- the interface ----
def test_header_and_renderer_have_the_interface():
    from capsaicin_amd import capi
    header = open(os.path.join(ROOT, "include", "capsaicin_hip.h")).read()
    for fn in ("cap_winding_instances", "cap_winding_instances_info", "cap_winding_instances_readback", "cap_objects_readback"):
        assert re.search(r"^int %s\(CapContext\* ctx" % fn, header, re.M), "%s is declared" % fn
        assert fn in capi.SYMBOLS
    assert "typedef struct CapWindingInstancesInfo" in header
    for method in ("winding_instances", "winding_instances_info", "winding_instances_tables", "objects_readback"):
        assert callable(getattr(capi.Renderer, method, None)), "Renderer.%s" % method
    import inspect
    sig = inspect.signature(capi.Renderer.signed_distance_instances)
    assert sig.parameters["sign"].default == "pseudonormal" and sig.parameters["beta"].default == 2.0
    assert C_size(capi.WindingInstancesInfo) == 160


def C_size(t):
    import ctypes
    return ctypes.sizeof(t)
