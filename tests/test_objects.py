"""Objects (cap_objects_set, cap_objects_info, cap_instances_set_ex) without a GPU: the header's structs and signatures, the exports
and the binding, the argument errors that need no device, and the brute force of tests/object_support.py on hand-computed answers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi
from instance_support import bits, f32, translations
from object_support import MISS, concat, expected, object_hits, object_occlusion, scene_triangles, single_triangle, triangle_ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cap_objects_set", "cap_objects_info", "cap_instances_set_ex")


def test_header_structs_and_signatures_compile(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "objects.c"
    src.write_text("""#include <stddef.h>
#include "capsaicin_hip.h"
_Static_assert(sizeof(CapObjectRange) == 8, "CapObjectRange");
_Static_assert(sizeof(CapObjectInfo) == 48, "CapObjectInfo");
_Static_assert(offsetof(CapObjectInfo, bounds_lo) == 16 && offsetof(CapObjectInfo, builder) == 40, "CapObjectInfo layout");
_Static_assert(sizeof(CapObjectsInfo) == 24 && offsetof(CapObjectsInfo, ms) == 16, "CapObjectsInfo");
_Static_assert(CAP_OBJECT_MAX_COUNT == 4096u, "CAP_OBJECT_MAX_COUNT");
_Static_assert(sizeof(CapInstanceDesc) == 64 && sizeof(((CapInstanceDesc*)0)->reserved) == 12, "CapInstanceDesc is as it was");
int (*const set)(CapContext*, const CapObjectRange*, uint32_t, CapObjectsInfo*) = cap_objects_set;
int (*const info)(CapContext*, CapObjectInfo*, uint32_t, uint32_t*) = cap_objects_info;
int (*const set_ex)(CapContext*, const CapInstanceDesc*, const uint32_t*, uint32_t, uint32_t, CapInstancesInfo*) = cap_instances_set_ex;
int (*const set_plain)(CapContext*, const CapInstanceDesc*, uint32_t, uint32_t, CapInstancesInfo*) = cap_instances_set;
static const CapObjectRange range = {.first_mesh = 0, .mesh_count = 1};
static const CapObjectsInfo all = {.count = 0, .triangles = 0, .nodes = 0, .max_depth = 0, .ms = 0.0};
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "objects.o")])


def test_entry_points_are_exported_and_bound(native_lib):
    for name in NEW:
        assert hasattr(native_lib, name), name
        assert name in capi.SYMBOLS, name
    assert ctypes.sizeof(capi.ObjectRange) == 8 and capi.OBJECT_RANGE_DTYPE.itemsize == 8
    assert ctypes.sizeof(capi.ObjectInfo) == 48 and capi.OBJECT_INFO_DTYPE.itemsize == 48
    assert capi.ObjectInfo.bounds_lo.offset == 16 and capi.ObjectInfo.builder.offset == 40
    assert capi.OBJECT_INFO_DTYPE.fields["bounds_lo"][1] == 16 and capi.OBJECT_INFO_DTYPE.fields["builder"][1] == 40
    assert ctypes.sizeof(capi.ObjectsInfo) == 24 and capi.ObjectsInfo.ms.offset == 16
    assert capi.OBJECT_MAX_COUNT == 4096
    for method in ("set_objects", "objects_info", "set_instances"):
        assert callable(getattr(capi.Renderer, method)), method
    import inspect
    assert "objects" in inspect.signature(capi.Renderer.set_instances).parameters


def test_null_context_errors_name_their_function(native_lib):
    r = (capi.ObjectRange * 1)()
    assert native_lib.cap_objects_set(None, r, 1, None) != 0
    assert b"cap_objects_set: ctx is NULL" in native_lib.cap_last_error()
    assert native_lib.cap_objects_info(None, None, 0, None) != 0
    assert b"cap_objects_info: ctx is NULL" in native_lib.cap_last_error()
    d = (capi.InstanceDesc * 1)()
    assert native_lib.cap_instances_set_ex(None, d, None, 1, 0, None) != 0
    assert b"cap_instances_set_ex: ctx is NULL" in native_lib.cap_last_error()
    assert native_lib.cap_instances_set(None, d, 1, 0, None) != 0
    assert b"cap_instances_set: ctx is NULL" in native_lib.cap_last_error()


def _ray(o, d, tmin=0.0, tmax=np.inf):
    return np.array([*o, tmin, *d, tmax], f32)


def _quad(z):
    """the square [0, 1]^2 in the plane z as one mesh of two triangles (normal +z)"""
    P = np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]], f32)
    N, T = np.tile(f32([0, 0, 1]), (4, 1)), np.zeros((4, 2), f32)
    return (P, N, T, np.array([0, 1, 2, 0, 2, 3], np.uint32), np.array([[4, 0, 6, 0, 0, 0xFFFFFFFF, 0, 0]], np.uint32))


def test_concat_and_triangle_ranges():
    arrays, ranges = concat([_quad(0.0), single_triangle(), _quad(2.0)])
    assert ranges.tolist() == [[0, 1], [1, 1], [2, 1]]
    assert arrays[4][:, 1].tolist() == [0, 4, 7] and arrays[4][:, 3].tolist() == [0, 6, 9] and arrays[4][:, 4].tolist() == [0, 1, 2]
    assert triangle_ranges(arrays[4], ranges).tolist() == [[0, 2], [2, 1], [3, 2]]
    assert triangle_ranges(arrays[4], [[1, 2], [0, 1]]).tolist() == [[2, 3], [0, 2]]
    tris = scene_triangles(arrays)
    assert tris.shape == (5, 3, 3) and np.all(tris[3:, :, 2] == 2.0) and np.array_equal(tris[2], single_triangle()[0])


def test_brute_force_known_answers():
    """Two objects -- object 0 the quad in z = 0 (triangles 0, 1), object 1 the quad in z = 2 (triangles 2, 3) -- and three
    instances: 0 shows object 0 as it is, 1 shows object 1 moved down by 1 (so in the plane z = 1), 2 shows object 0 moved up by 1
    (also in the plane z = 1)."""
    arrays, ranges = concat([_quad(0.0), _quad(2.0)])
    tris, tr = scene_triangles(arrays), triangle_ranges(arrays[4], ranges)
    mot = np.array([0, 0, 1, 1])
    M = translations([[0, 0, 0], [0, 0, -1], [0, 0, 1]])
    W = translations([[0, 0, 0], [0, 0, 1], [0, 0, -1]])  # exact inverses
    objects = np.array([0, 1, 0])
    live = np.ones(3, bool)
    assert M.shape == W.shape
    # straight down from z = 5 through (0.75, 0.25): triangle 0 of each quad (y <= x)
    down = _ray((0.75, 0.25, 5), (0, 0, -1))
    h = object_hits(down, W, live, None, objects, tris, tr, mot)
    # instance 0 of object 0 does NOT report object 1's triangle 2, although the ray crosses the plane z = 2 "inside" instance 0's
    # frame: the hits are the two in the plane z = 1 (t = 4), tied, instance 1 (object 1, triangle 2) before instance 2 (object 0,
    # triangle 0) by the instance index although its triangle id is the larger one, then z = 0 (t = 5)
    assert [(round(float(t), 4), i, g) for t, _, _, i, g in h] == [(4.0, 1, 2), (4.0, 2, 0), (5.0, 0, 0)]
    assert bits(h[0][0]) == bits(h[1][0]), "the tie is an exact one: equal float32 t from different objects' triangles"
    rec, inst = closest_record_of(h, down)
    assert inst == 1 and rec[3] == 2 and rec[0] == bits(h[0][0])
    # without the object table the same three instances show both quads each: six hits, the first at z = 3 (t = 2)
    from instance_support import instanced_hits
    flat = instanced_hits(down, W, live, None, tris, mot)
    assert [(round(float(t), 4), i, g) for t, _, _, i, g in flat] == [(2.0, 2, 2), (3.0, 0, 2), (4.0, 1, 2), (4.0, 2, 0), (5.0, 0, 0), (6.0, 1, 0)]
    # the other order of objects in the table: the tie still goes to the lower INSTANCE
    # instance 1 shows object 0 (plane z = -1), instance 2 object 1 (plane z = 3)
    h2 = object_hits(down, W, live, None, np.array([0, 0, 1]), tris, tr, mot)
    assert [(round(float(t), 4), i, g) for t, _, _, i, g in h2] == [(2.0, 2, 2), (5.0, 0, 0), (6.0, 1, 0)]
    # masks: instance mask & mesh mask & inclusion, per object; occlusion is the OR over the objects
    mm = np.array([0x01, 0x02], np.uint8)
    assert [(i, g) for *_, i, g in object_hits(down, W, live, [0xFF, 0x01, 0xFF], objects, tris, tr, mot, mm)] == [(2, 0), (0, 0)]
    assert [(i, g) for *_, i, g in object_hits(down, W, live, None, objects, tris, tr, mot, mm, mask=0x02)] == [(1, 2)]
    assert object_occlusion(down, W, live, None, objects, tris, tr, mot, mm, mask=0x02) == 1
    assert object_occlusion(down, W, live, [0xFF, 0x01, 0xFF], objects, tris, tr, mot, mm, mask=0x02) == 0
    assert object_hits(down, W, np.zeros(3, bool), None, objects, tris, tr, mot) == []
    # cull: both quads face +z, the ray comes from above
    assert len(object_hits(down, W, live, None, objects, tris, tr, mot, cull="back")) == 3
    assert object_hits(down, W, live, None, objects, tris, tr, mot, cull="front") == []
    # expected(): records, instances and occlusion words, candidates prefiltered per object
    rays = np.stack([down, _ray((0.75, 0.25, 5), (0, 0, 1)), _ray((0.25, 0.75, 1.5), (0, 0, -1))])
    rec, inst, occ, lists = expected(rays, W, live, None, objects, tris, tr, mot)
    assert inst.tolist() == [1, MISS, 1] and occ.tolist() == [1, 0, 1]
    assert rec[0, 3] == 2 and rec[0, 0] == bits(h[0][0]) and lists[0] == h
    assert rec[1, 3] == MISS and rec[2, 3] == 3 and round(float(rec.view(f32)[2, 0]), 4) == 0.5 and lists[2][1][3:] == (2, 1)


def closest_record_of(hits, ray):
    from instance_support import closest_record
    return closest_record(hits, ray[7])
