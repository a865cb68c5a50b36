"""Vertex updates and refit (cap_scene_update_vertices / cap_bvh_refit) without a GPU: the CapRefitInfo layout of the C header and of
the Python binding agree, the entry points are exported, and Renderer.update_vertices checks its arrays before any call."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refit_info_layout():
    assert ctypes.sizeof(capi.RefitInfo) == 24
    assert (capi.RefitInfo.ms.offset, capi.RefitInfo.expected_node_visits.offset, capi.RefitInfo.expected_node_visits_built.offset) == (0, 8, 16)
    assert capi.VERTICES_DEVICE == 1


def test_header_refit_layout_compiles(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "refit_layout.c"
    src.write_text("""#include <stddef.h>
#include "capsaicin_hip.h"
_Static_assert(sizeof(CapRefitInfo) == 24, "CapRefitInfo");
_Static_assert(offsetof(CapRefitInfo, expected_node_visits) == 8 && offsetof(CapRefitInfo, expected_node_visits_built) == 16, "fields");
_Static_assert(CAP_VERTICES_DEVICE == 1, "flag");
int (*const update)(CapContext*, const float*, const float*, const float*, uint32_t) = cap_scene_update_vertices;
int (*const refit)(CapContext*, CapRefitInfo*) = cap_bvh_refit;
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "refit_layout.o")])


def test_entry_points_are_exported(native_lib):
    for name in ("cap_scene_update_vertices", "cap_bvh_refit"):
        assert hasattr(native_lib, name)
        assert name in capi.SYMBOLS
    assert capi.SYMBOLS["cap_bvh_refit"][1][1] == ctypes.POINTER(capi.RefitInfo)


def test_null_context_is_an_argument_error(native_lib):
    assert native_lib.cap_scene_update_vertices(None, None, None, None, 0) == 1  # CAP_ERR_INVALID_ARG
    assert native_lib.cap_bvh_refit(None, None) == 1


def _renderer(vertex_count):
    r = capi.Renderer.__new__(capi.Renderer)  # (no context: the checks come first)
    r.ctx, r.device, r._vertex_count = None, 0, vertex_count
    return r


@pytest.mark.parametrize("shape", [(4, 3), (12,)])
def test_update_vertices_accepts_both_shapes(shape):
    ptrs, flags, keep = capi.vertex_update_args(4, positions=np.zeros(shape, np.float32), texcoords=np.zeros((4, 2), np.float32))
    assert flags == 0 and ptrs[1] is None and ptrs[0] is not None and ptrs[2] is not None and len(keep) == 2


@pytest.mark.parametrize("kw", [dict(positions=np.zeros((5, 3), np.float32)), dict(normals=np.zeros((4, 2), np.float32)),
                                dict(texcoords=np.zeros((4, 3), np.float32)), dict(positions=np.zeros((4, 3, 1), np.float32)),
                                dict(texcoords=np.zeros(9, np.float32))])
def test_update_vertices_rejects_shapes(kw):
    with pytest.raises(capi.CapError, match="shape"):
        _renderer(4).update_vertices(**kw)


@pytest.mark.parametrize("dtype", [np.float64, np.float16, np.int32])
def test_update_vertices_rejects_dtypes(dtype):
    with pytest.raises(capi.CapError, match="float32"):
        _renderer(4).update_vertices(positions=np.zeros((4, 3), dtype))


def test_update_vertices_rejects_lists():
    with pytest.raises(capi.CapError, match="numpy arrays or torch tensors"):
        _renderer(1).update_vertices(positions=[[0.0, 0.0, 0.0]])


def test_update_vertices_rejects_mixed_kinds():
    torch = pytest.importorskip("torch")
    with pytest.raises(capi.CapError, match="mixing"):
        _renderer(4).update_vertices(positions=np.zeros((4, 3), np.float32), normals=torch.zeros((4, 3)))


def test_update_vertices_rejects_host_tensors():
    torch = pytest.importorskip("torch")
    with pytest.raises(capi.CapError, match="on the GPU"):
        _renderer(4).update_vertices(positions=torch.zeros((4, 3)))
    with pytest.raises(capi.CapError, match="float32"):
        capi.vertex_update_args(4, normals=torch.zeros((4, 3), dtype=torch.float64))
