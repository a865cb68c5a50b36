"""Ray queries (cap_trace_rays / cap_trace_occlusion) without a GPU: the record layouts of the C header and of the Python binding
agree, the entry points are exported, and the host-side id mapping is the mesh-table walk."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_layouts_match_the_header():
    assert ctypes.sizeof(capi.RayDesc) == 32 and ctypes.sizeof(capi.Hit) == 16
    assert (capi.RayDesc.origin.offset, capi.RayDesc.tmin.offset, capi.RayDesc.direction.offset, capi.RayDesc.tmax.offset) == (0, 12, 16, 28)
    assert (capi.Hit.t.offset, capi.Hit.u.offset, capi.Hit.v.offset, capi.Hit.triangle.offset) == (0, 4, 8, 12)


def test_header_layouts_compile(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "layout.c"
    src.write_text("""#include <stddef.h>
#include "capsaicin_hip.h"
_Static_assert(sizeof(CapRayDesc) == 32, "CapRayDesc");
_Static_assert(sizeof(CapHit) == 16, "CapHit");
_Static_assert(offsetof(CapRayDesc, tmin) == 12 && offsetof(CapRayDesc, direction) == 16 && offsetof(CapRayDesc, tmax) == 28, "RayDesc");
_Static_assert(offsetof(CapHit, u) == 4 && offsetof(CapHit, v) == 8 && offsetof(CapHit, triangle) == 12, "CapHit fields");
int (*const trace)(CapContext*, const CapRayDesc*, uint64_t, CapHit*, uint32_t) = cap_trace_rays;
int (*const occl)(CapContext*, const CapRayDesc*, uint64_t, uint32_t*, uint32_t) = cap_trace_occlusion;
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout.o")])


def test_entry_points_are_exported(native_lib):
    for name in ("cap_trace_rays", "cap_trace_occlusion"):
        assert hasattr(native_lib, name)
        assert name in capi.SYMBOLS


def test_hit_triangles_reads_the_id_bits():
    hits = np.zeros((3, 4), np.float32)
    hits[:, 3] = np.array([0, 123456, 0xFFFFFFFF], np.uint32).view(np.float32)
    assert hits.view(np.uint32)[2, 3] == capi.MISS
    ids = capi.hit_triangles(hits)
    assert ids.dtype == np.int64 and list(ids) == [0, 123456, capi.MISS]


def test_triangle_to_instance_primitive_walks_the_mesh_table():
    """Ids count mesh-table order then primitive order, whatever the meshes' first_index_offset says."""
    r = capi.Renderer.__new__(capi.Renderer)  # (no context: the mapping is host-side)
    r.ctx = None
    meshes = np.zeros((3, 8), np.uint32)
    meshes[:, 2] = (6, 9, 3)      # index_count: 2, 3 and 1 triangles
    meshes[:, 3] = (9, 0, 15)     # first_index_offset out of order
    r._set_mesh_table(meshes)
    inst, prim = r.triangle_to_instance_primitive(np.array([0, 1, 2, 3, 4, 5, 6, capi.MISS], np.int64))
    assert list(inst) == [0, 0, 1, 1, 1, 2, capi.MISS, capi.MISS]
    assert list(prim) == [0, 1, 0, 1, 2, 0, capi.MISS, capi.MISS]
