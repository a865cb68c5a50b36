"""Ray flags and instance masks of the ray queries (cap_trace_*_ex) without a GPU: the header's constants, struct and signatures, the
exports and the binding, and the brute-force helpers of the GPU tests on hand-computed answers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi
from filter_support import (MISS, all_hits, bits, closest_record, faced_hits, facing, filtered_hits, filtered_occlusion,
                            mesh_of_triangles, occludes, stacked_quads_meshes)
from multi_hit_support import stacked_quads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cap_scene_set_instance_masks", "cap_trace_rays_ex", "cap_trace_occlusion_ex", "cap_trace_rays_multi_ex")


def test_header_flags_struct_and_signatures_compile(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "filter.c"
    src.write_text("""#include "capsaicin_hip.h"
_Static_assert(CAP_RAY_FLAG_ACCEPT_FIRST_HIT == 0x04, "RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH");
_Static_assert(CAP_RAY_FLAG_CULL_BACK_FACING == 0x10, "RAY_FLAG_CULL_BACK_FACING_TRIANGLES");
_Static_assert(CAP_RAY_FLAG_CULL_FRONT_FACING == 0x20, "RAY_FLAG_CULL_FRONT_FACING_TRIANGLES");
_Static_assert(sizeof(CapTraceOptions) == 16, "CapTraceOptions");
_Static_assert(sizeof(((CapTraceOptions*)0)->reserved) == 8, "reserved[2]");
int (*const masks)(CapContext*, const uint8_t*, uint32_t) = cap_scene_set_instance_masks;
int (*const closest)(CapContext*, const CapRayDesc*, uint64_t, CapHit*, const CapTraceOptions*) = cap_trace_rays_ex;
int (*const occlusion)(CapContext*, const CapRayDesc*, uint64_t, uint32_t*, const CapTraceOptions*) = cap_trace_occlusion_ex;
int (*const multi)(CapContext*, const CapRayDesc*, uint64_t, uint32_t, CapHit*, uint32_t*, uint32_t, const CapTraceOptions*) =
    cap_trace_rays_multi_ex;
static const CapTraceOptions zero = {0};
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "filter.o")])


def test_entry_points_are_exported_and_bound(native_lib):
    import ctypes
    for name in NEW:
        assert hasattr(native_lib, name), name
        assert name in capi.SYMBOLS, name
    R = capi.Renderer
    assert (R.RAY_FLAG_ACCEPT_FIRST_HIT, R.RAY_FLAG_CULL_BACK_FACING, R.RAY_FLAG_CULL_FRONT_FACING) == (0x04, 0x10, 0x20)
    assert ctypes.sizeof(capi.TraceOptions) == 16 and capi.TraceOptions.instance_mask.offset == 4
    # the defaults are the plain calls: no options struct at all
    assert R.trace_options(R, None, None, False) is None
    o = R.trace_options(R, "front", 0x21, True)
    assert (o.ray_flags, o.instance_mask, tuple(o.reserved)) == (0x24, 0x21, (0, 0))
    assert R.trace_options(R, "back").ray_flags == 0x10
    with pytest.raises(capi.CapError):
        R.trace_options(R, "both")


def _ray(o, d, tmin=0.0, tmax=np.inf):
    return np.array([*o, tmin, *d, tmax], np.float32)


def test_facing_known_answers():
    """The quads' n = e1 x e2 = (0, 0, 1): a +z ray travels along n and sees back faces, a -z ray front faces.  Swapping v1, v2
    flips the sign; a ray in the plane has det = 0.  For every hit the oracle reports, facing is non-zero."""
    _, tris = stacked_quads(4, 0.25)
    up, down = _ray((0.3, 0.7, -1.0), (0, 0, 1)), _ray((0.3, 0.7, 9.0), (0, 0, -1))
    for t in tris:
        assert facing(up, t) == -1 and facing(down, t) == 1
        assert facing(up, t[[0, 2, 1]]) == 1 and facing(down, t[[0, 2, 1]]) == -1
        assert facing(_ray((0.3, 0.7, -1.0), (1, 0.5, 0)), t) == 0
    rng = np.random.default_rng(3)
    T = rng.normal(size=(60, 3, 3)).astype(np.float32)
    n_hits = 0
    for _ in range(200):
        o = rng.normal(size=3) * 3
        r = _ray(o, T[rng.integers(60)].mean(0) - o + rng.normal(size=3) * 0.05)
        for *_, g in all_hits(r, T):
            n_hits += 1
            f = facing(r, T[g])
            assert f != 0 and facing(r, T[g][[0, 2, 1]]) == -f
            # float64 agrees wherever it is far from zero (the helper itself is exact, this only guards the transcription)
            d64 = -np.dot(r[4:7].astype(np.float64), np.cross(T[g, 1].astype(np.float64) - T[g, 0], T[g, 2].astype(np.float64) - T[g, 0]))
            if abs(d64) > 1e-4:
                assert f == np.sign(d64)
    assert n_hits > 200


def test_filtered_hits_on_stacked_quads():
    arrays, tris = stacked_quads_meshes(40, 0.25)
    _, same = stacked_quads(40, 0.25)
    assert np.array_equal(tris, same)  # the same triangles, one mesh per quad
    mot = mesh_of_triangles(arrays[4])
    assert list(mot[:6]) == [0, 0, 1, 1, 2, 2] and len(mot) == 80
    up, down = _ray((0.3, 0.7, -1.0), (0, 0, 1)), _ray((0.3, 0.7, 10.5), (0, 0, -1))
    ids = lambda h: [g for *_, g in h]
    full = [2 * i + 1 for i in range(40)]
    # +z sees back faces only: cull back drops everything, cull front nothing; -z the other way round
    assert ids(filtered_hits(up, tris, mot, None)) == full
    assert ids(filtered_hits(up, tris, mot, None, "back")) == [] and ids(filtered_hits(up, tris, mot, None, "front")) == full
    assert ids(filtered_hits(down, tris, mot, None, "front")) == [] and ids(filtered_hits(down, tris, mot, None, "back")) == full[::-1]
    # masks: every other quad, one quad, nothing
    masks = np.where(np.arange(40) % 2 == 0, 0x01, 0x02).astype(np.uint8)
    assert ids(filtered_hits(up, tris, mot, masks, None, 0x01)) == [2 * i + 1 for i in range(0, 40, 2)]
    assert ids(filtered_hits(up, tris, mot, masks, None, 0x02)) == [2 * i + 1 for i in range(1, 40, 2)]
    assert ids(filtered_hits(up, tris, mot, masks, None, 0x03)) == full and ids(filtered_hits(up, tris, mot, masks, None, None)) == full
    assert ids(filtered_hits(up, tris, mot, masks, None, 0x04)) == []
    one = np.zeros(40, np.uint8)
    one[7] = 0x80
    assert ids(filtered_hits(up, tris, mot, one, "front", 0xFF)) == [15]
    # the closest record skips a rejected nearer hit, and is the miss record when nothing passes
    rec = closest_record(filtered_hits(up, tris, mot, one, None, 0x80), up[7])
    assert bits(rec)[3] == 15 and np.isclose(rec[0], 1.0 + 0.25 * 7, rtol=1e-6, atol=0)  # (the contract's reciprocal is not exact)
    miss = closest_record(filtered_hits(up, tris, mot, one, "back", 0x80), up[7])
    assert bits(miss)[3] == MISS and np.isinf(miss[0]) and miss[1] == 0 and miss[2] == 0
    # the shared diagonal: both triangles of a quad have the same facing, so a cull keeps both or neither
    diag = _ray((0.5, 0.5, -1.0), (0, 0, 1))
    f = faced_hits(diag, tris)
    assert [h[3] for h in f] == list(range(80)) and all(h[4] == -1 for h in f)
    assert ids(filtered_hits(diag, tris, mot, None, "front", faced=f)) == list(range(80))
    assert ids(filtered_hits(diag, tris, mot, None, "back", faced=f)) == []
    assert ids(filtered_hits(diag, tris, mot, masks, "front", 0x02, faced=f)) == [g for g in range(80) if (g // 2) % 2 == 1]


def test_occlusion_helper_and_flipped_quads():
    """occludes() is the oracle's divided test wherever no hit lies at an interval end; every third quad wound the other way shows
    both facings to one vertical ray, and the filtered occlusion follows the filtered hit set."""
    rng = np.random.default_rng(8)
    T = rng.normal(size=(40, 3, 3)).astype(np.float32)
    n = 0
    for _ in range(60):
        o = rng.normal(size=3) * 3
        r = _ray(o, T[rng.integers(40)].mean(0) - o, 0.0, np.inf)
        hit = {g for *_, g in all_hits(r, T)}
        assert {g for g in range(40) if occludes(r, T[g])} == hit
        n += len(hit)
    assert n > 60
    arrays, tris = stacked_quads_meshes(6, 0.25, flip_every=3)
    mot = mesh_of_triangles(arrays[4])
    up = _ray((0.3, 0.7, -1.0), (0, 0, 1))
    assert [facing(up, t) for t in tris] == [-1, -1, -1, -1, 1, 1] * 2
    ids = lambda h: [g for *_, g in h]
    assert ids(filtered_hits(up, tris, mot, None, "back")) == [5, 11] and ids(filtered_hits(up, tris, mot, None, "front")) == [1, 3, 7, 9]
    only2 = np.array([0, 0, 1, 0, 0, 0], np.uint8)
    assert filtered_occlusion(up, tris, mot, only2, None, 1) == 1 and filtered_occlusion(up, tris, mot, only2, "front", 1) == 0
    assert filtered_occlusion(up, tris, mot, only2, "back", 1) == 1 and filtered_occlusion(up, tris, mot, only2, "back", 2) == 0
    cut = _ray((0.3, 0.7, -1.0), (0, 0, 1), 0.0, 1.4)  # z in (-1, 0.4): quads 0 and 1 only, both back-facing
    assert filtered_occlusion(cut, tris, mot, None, "front") == 1 and filtered_occlusion(cut, tris, mot, None, "back") == 0
