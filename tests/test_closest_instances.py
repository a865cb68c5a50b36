"""Closest-point queries over instances (cap_closest_instances) without a GPU: the header's prototype, the export and the binding; the
numpy reference (closest_instances_support.py) pinned by hand, its ties, masks, radii and identities, and its float64 twin; the debug
entry cap_debug_closest_instance_bound -- g against numpy's SVD, W, and that the shipped skip predicate never skips the box of a
triangle at its own contract distance; the address checks of the call's three arrays."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_instances_support import (MISS, affine, bits, bound, closest_instances, flat_record, identity, live_of, near_translations,
                                       pair_valid, triangles_of, world_hull_points, world_points_near, world_records)
from closest_point_support import around, closest, needles, queries, soup, sphere
from instance_support import extreme_transforms, flatten, grid_scene, regular_transforms, rotation, translations
from multi_hit_support import stacked_quads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID_ARG = 0, 1


def test_header_prototype_compiles(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "closest_inst.c"
    src.write_text("""#include "capsaicin_hip.h"
int (*const closest)(CapContext*, const CapPointDesc*, uint64_t, CapClosest*, uint32_t*, const CapTraceOptions*) = cap_closest_instances;
int (*const dbg)(const float*, const float*, const float*, const float*, float, float*, float*, float*, float*, uint32_t*) =
    cap_debug_closest_instance_bound;
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "closest_inst.o")])


def test_entry_points_are_exported_and_bound(native_lib):
    assert hasattr(native_lib, "cap_closest_instances") and hasattr(native_lib, "cap_debug_closest_instance_bound")
    assert len(capi.SYMBOLS["cap_closest_instances"][1]) == 6 and len(capi.SYMBOLS["cap_debug_closest_instance_bound"][1]) == 10
    assert callable(capi.Renderer.closest_instances)
    assert native_lib.cap_closest_instances(None, None, 0, None, None, None) == ERR_INVALID_ARG
    assert b"cap_closest_instances: ctx is NULL" in native_lib.cap_last_error()
    assert native_lib.cap_debug_closest_instance_bound(None, None, None, None, 0.0, None, None, None, None, None) == ERR_INVALID_ARG


# ---- the reference pinned by hand ----
UNIT = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
STRETCH = affine(np.diag([10.0, 1.0, 1.0]), (2, 3, 4))  # the world triangle (2, 3, 4), (12, 3, 4), (2, 4, 4)
# point, feature, (u, v), closest point, dist2: every value exact in binary32
FEATURES = [((4.5, 3.25, 5.0), 0, (0.25, 0.25), (4.5, 3.25, 4), 1.0),
            ((7.0, 2.0, 4.0), 1, (0.5, 0.0), (7, 3, 4), 1.0),
            ((7.5, 8.5, 4.0), 2, (0.5, 0.5), (7, 3.5, 4), 25.25),
            ((1.0, 3.5, 4.0), 3, (0.0, 0.5), (2, 3.5, 4), 1.0),
            ((1.0, 2.0, 4.0), 4, (0.0, 0.0), (2, 3, 4), 2.0),
            ((13.0, 2.5, 4.0), 5, (1.0, 0.0), (12, 3, 4), 1.25),
            ((1.5, 5.0, 4.0), 6, (0.0, 1.0), (2, 4, 4), 1.25)]


def test_world_record_known_answers():
    v0w, e1w, e2w = world_records([STRETCH], UNIT)
    assert v0w[0, 0].tolist() == [2, 3, 4] and e1w[0, 0].tolist() == [10, 0, 0] and e2w[0, 0].tolist() == [0, 1, 0]
    # single roundings in the contract's order: ((a + b) + c) + t, not the float64 value rounded once
    M = np.float32([[[0.1, 0.2, 0.3, 0.7], [0, 1, 0, 0], [0, 0, 1, 0]]])
    t = np.float32([[[3, 5, 7], [4, 5, 7], [3, 6, 7]]])
    f = np.float32
    want = f(f(f(f(f(0.1) * f(3)) + f(f(0.2) * f(5))) + f(f(0.3) * f(7))) + f(0.7))
    assert world_records(M, t)[0][0, 0, 0] == want


@pytest.mark.parametrize("case", FEATURES, ids=[str(c[1]) for c in FEATURES])
def test_each_feature_under_an_anisotropic_transform(case):
    p, feature, (u, v), point, d2 = case
    rec, inst = closest_instances(queries([p]), [STRETCH], UNIT)
    assert inst.tolist() == [0]
    assert rec[0, 0:3].tolist() == list(map(float, point)) and rec[0, 3] == d2 and (rec[0, 4], rec[0, 5]) == (u, v)
    assert bits(rec)[0, 6:8].tolist() == [0, feature]


def test_nearest_in_world_space_is_not_nearest_in_object_space():
    """diag(10, 1, 1): triangle 0 is 1 away along x in object space and 10 in world space; triangle 1 is 2.5 away along y in both"""
    tris = np.float32([[[1, 0, 0], [2, 1, 0], [2, -1, 0]], [[0, 2.5, 0], [1, 3.5, 0], [-1, 3.5, 0]]])
    M = affine(np.diag([10.0, 1.0, 1.0]))
    q = queries([(0, 0, 0)])
    rec, inst, table = closest_instances(q, [M], tris, with_table=True)
    assert table[0, 0].tolist() == [100.0, 6.25]
    assert bits(rec)[0, 6] == 1 and rec[0, 3] == 6.25 and inst[0] == 0
    flat, ftable = closest(q, tris)
    assert ftable[0].tolist() == [1.0, 6.25] and bits(flat)[0, 6] == 0


# ---- ties, inert and masked instances, radius, degenerate points ----
def test_ties_inert_and_masked_instances():
    _, tris = stacked_quads(6, 0.25)
    shift = affine(np.eye(3), (0, 0, 0.25))
    nan = identity()[0].copy()
    nan[1, 1] = np.nan
    M = np.stack([nan, identity()[0], identity()[0], shift, np.zeros((3, 4), np.float32)])
    live = live_of(M)
    assert live.tolist() == [False, True, True, True, False]
    q = queries([(0.5, 0.25, 0.125), (0.25, 0.5, 0.375), (0.5, 0.5, -1.0)])
    rec, inst, table = closest_instances(q, M, tris, pair_valid(5, len(tris), live), with_table=True)
    assert (inst == 1).all(), "coincident instances tie and the lower live one wins"
    best = rec[:, 3]
    with np.errstate(invalid="ignore"):
        tied = (table[:, 1:4] == best[:, None, None]).sum((1, 2))
    assert (tied >= 4).all() and (table[:, 3] == best[:, None]).any(), "ties within and across instances"
    # masked out: instance 1 by its own mask, then everything by the call's mask
    masks = np.uint32([0xFF, 0x02, 0x01, 0x01, 0xFF])
    rec2, inst2 = closest_instances(q, M, tris, pair_valid(5, len(tris), live, masks, None, 0x01))
    assert (inst2 == 2).all() and np.array_equal(bits(rec2), bits(rec))
    rec3, inst3 = closest_instances(q, M, tris, pair_valid(5, len(tris), live, masks, None, 0x04))
    assert (inst3 == -1).all() and (bits(rec3)[:, 6] == MISS).all() and np.isinf(rec3[:, 3]).all()
    # a mesh mask that leaves only the upper triangle of every quad
    tri_masks = np.where(np.arange(len(tris)) % 2 == 1, 0xFF, 0x00)
    rec4, _ = closest_instances(q, M, tris, pair_valid(5, len(tris), live, None, tri_masks))
    assert (bits(rec4)[:, 6] % 2 == 1).all()


def test_radius_at_below_and_without_and_degenerate_points():
    rng = np.random.default_rng(3)
    tris = soup(rng, 40, edge=0.2)
    M = regular_transforms(6)
    q = queries(world_hull_points(rng, M, tris, 64))
    free, inst = closest_instances(q, M, tris)
    assert (inst >= 0).all()
    at = np.sqrt(free[:, 3])
    hits = {}
    for name, radius in (("at", at), ("below", np.nextafter(at, np.float32(0))), ("inf", np.float32(np.inf))):
        q[:, 3] = radius
        rec, i = closest_instances(q, M, tris)
        hits[name] = i >= 0
        assert np.array_equal(bits(rec[i >= 0]), bits(free[i >= 0])), "a radius does not change a hit"
        assert (rec[i < 0, 3] == q[i < 0, 3] * q[i < 0, 3]).all() and (bits(rec)[i < 0, 6] == MISS).all(), "the miss record carries r2"
    assert hits["inf"].all() and 0 < hits["at"].sum() and hits["below"].sum() < hits["at"].sum()
    bad = queries([(np.nan, 0, 0), (0, np.inf, 0), (0, 0, 0), (1, 1, 1)])
    bad[2, 3], bad[3, 3] = -1.0, np.nan
    rec, i = closest_instances(bad, M, tris)
    miss = np.zeros(8, np.uint32)
    miss[6] = MISS
    assert (i == -1).all() and (bits(rec) == miss).all()


# ---- the three identities, on the reference ----
def test_identity_instance_is_the_flat_query():
    rng = np.random.default_rng(5)
    tris = soup(rng, 60, edge=0.3)
    q = queries(around(rng, tris, 96, 0.5))
    q[48:, 3] = 0.3
    rec, inst = closest_instances(q, identity(), tris)
    flat, _ = closest(q, tris)
    assert np.array_equal(bits(rec), bits(flat)) and ((inst == 0) == (bits(flat)[:, 6] != MISS)).all()


def test_grid_translations_are_the_flattened_scene():
    arrays, tris = grid_scene(12)
    T = len(tris)
    tr = np.float32([[0, 0, 0], [16, 0, 0], [0, 0, 0], [-32, 16, 48]])
    rng = np.random.default_rng(6)
    q = queries(rng.integers(-64 * 16, 64 * 16 + 1, (96, 3)) / 16.0)
    q[64:, 3] = 12.0
    rec, inst = closest_instances(q, translations(tr), tris)
    flat, _ = closest(q, triangles_of(flatten(arrays, tr)))
    assert np.array_equal(bits(flat_record(rec, inst, T)), bits(flat))
    assert (inst == 0).sum() > 0 and (inst == 2).sum() == 0 and (inst == 3).sum() > 0 and (inst == -1).sum() > 0


def test_power_of_two_scaling():
    rng = np.random.default_rng(7)
    tris = soup(rng, 60, edge=0.3)
    M = regular_transforms(6)
    q = queries(world_hull_points(rng, M, tris, 64), 8.0)
    rec, inst = closest_instances(q, M, tris)
    for k in (2, -3):
        s = np.float32(2.0 ** k)
        rec_s, inst_s = closest_instances(q * s, M * s, tris)
        assert np.array_equal(inst_s, inst) and np.array_equal(bits(rec_s)[:, 4:8], bits(rec)[:, 4:8])
        hit = inst >= 0
        assert np.array_equal(rec_s[hit, 0:3], rec[hit, 0:3] * s) and np.array_equal(rec_s[:, 3], rec[:, 3] * s * s)
    assert 0 < (inst >= 0).sum() < len(q), "hits and misses"


def test_uniform_scale_by_four_multiplies_dist2_by_sixteen():
    rng = np.random.default_rng(8)
    tris = soup(rng, 30, edge=0.3)
    q = queries(around(rng, tris, 32, 0.5))
    flat, _ = closest(q, tris)
    q4 = q.copy()
    q4[:, 0:3] *= 4
    rec, inst = closest_instances(q4, [affine(4.0 * np.eye(3))], tris)
    assert np.array_equal(rec[:, 3], flat[:, 3] * 16) and np.array_equal(bits(rec)[:, 4:8], bits(flat)[:, 4:8])


# ---- the float64 twin, tied to the shipped slack ----
def object_box(tris):
    return tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)


def test_float32_reference_against_its_float64_twin(native_lib):
    rng = np.random.default_rng(9)
    tris = soup(rng, 60, edge=0.2, min_shape=0.2)
    M = regular_transforms(24)
    q = queries(np.concatenate([world_hull_points(rng, M, tris, 24), world_points_near(rng, M, tris, 24, 1e-2)]))
    _, _, t32 = closest_instances(q, M, tris, with_table=True)
    _, _, t64 = closest_instances(q, M, tris, dtype=np.float64, with_table=True)
    lo, hi = object_box(tris)
    slack = np.array([[bound(M[i], lo, hi, p[0:3], 0.0, native_lib)["slack"] for i in range(len(M))] for p in q], np.float64)
    err = np.abs(np.sqrt(t32.astype(np.float64)) - np.sqrt(t64))
    worst = (err / slack[:, :, None]).max()
    print("largest |sqrt(d2_32) - sqrt(d2_64)| / slack_i(p): %.4f" % worst)
    assert worst <= 1.0


# ---- the debug entry ----
def test_g_is_a_tight_lower_bound_on_sigma_min(native_lib):
    Ms = np.concatenate([regular_transforms(48), extreme_transforms()[0]])
    must_be_inert = np.concatenate([np.zeros(48, bool), extreme_transforms()[1]])
    live = 0
    for M, inert in zip(Ms, must_be_inert):
        b = bound(M, (-1, -1, -1), (1, 1, 1), (0, 0, 0), 0.0, native_lib)
        if inert:
            assert b["g"] == 0 and not b["W"].any() and b["skip"] == 0
            continue
        if b["g"] == 0:
            continue  # beyond CAP_INSTANCE_MAX_CONDITION
        live += 1
        sv = np.linalg.svd(M[:, :3].astype(np.float64), compute_uv=False)
        assert 0 < b["g"] <= sv[-1], (M, b["g"], sv)
        if sv[0] / sv[-1] <= 100.0:
            assert b["g"] >= 0.99 * sv[-1], (M, b["g"], sv)
        inv = np.linalg.inv(np.vstack([M.astype(np.float64), [0, 0, 0, 1]]))[:3]
        assert np.all(np.abs(b["W"].astype(np.float64) - inv) <= 2.0 ** -24 * np.abs(inv) + 1e-12 * np.abs(inv).max())
        # Xw: no |coordinate| of the box's image exceeds it, nor does the translation
        corners = np.array([[(-1, 1)[(c >> k) & 1] for k in range(3)] for c in range(8)], np.float64)
        assert b["xw"] >= np.abs(corners @ M[:, :3].astype(np.float64).T + M[:, 3]).max() and b["xw"] >= np.abs(M[:, 3]).max()
    assert live >= 49


def assert_never_skipped(native_lib, M, tris, pts, what):
    """every (point, instance, triangle): the triangle's own float32 box, its contract dist2 as the best"""
    _, _, table = closest_instances(queries(pts), M, tris, with_table=True)
    lo, hi = tris.min(1), tris.max(1)
    n = 0
    for a, p in enumerate(pts):
        for i in range(len(M)):
            for g in range(len(tris)):
                d2 = table[a, i, g]
                if not np.isfinite(d2):
                    continue
                b = bound(M[i], lo[g], hi[g], p, d2, native_lib)
                assert b["g"] > 0 and b["skip"] == 0, (what, a, i, g, p.tolist(), float(d2), b)
                n += 1
    return n


BOUND_SCENES = ("regular", "translations near 4096", "points 1e5 away", "points within 1e-3", "needles", "sphere from its centre")


@pytest.mark.parametrize("name", BOUND_SCENES)
def test_the_bound_never_skips_a_candidate(native_lib, name):
    rng = np.random.default_rng(10)
    tris = soup(rng, 40, edge=0.2, min_shape=0.2)
    M = regular_transforms(12)
    if name == "regular":
        pts = np.concatenate([world_hull_points(rng, M, tris, 6), world_points_near(rng, M, tris, 6, 0.05)])
    elif name == "translations near 4096":
        M = near_translations(M)
        pts = np.concatenate([world_hull_points(rng, M, tris, 6), world_points_near(rng, M, tris, 6, 0.05)])
    elif name == "points 1e5 away":
        d = rng.normal(size=(10, 3))
        pts = (d / np.linalg.norm(d, axis=1, keepdims=True) * 1e5).astype(np.float32)
    elif name == "points within 1e-3":
        pts = world_points_near(rng, M, tris, 12, 1e-3)
    elif name == "needles":
        tris = needles(rng, 40, 0.2, 1e4)
        pts = np.concatenate([world_hull_points(rng, M, tris, 4), world_points_near(rng, M, tris, 8, 1e-3)])
    else:
        tris = sphere(rows=8, cols=8)
        R = rotation(rng)
        M = np.stack([affine(R @ np.diag([1.0, 30.0, 90.0]) @ R.T, (3, -2, 5))])
        pts = (np.float64([3, -2, 5]) + np.concatenate([np.zeros((1, 3)), rng.normal(size=(20, 3)) * 1e-3, rng.normal(size=(10, 3)) * 1e-6])).astype(np.float32)
    assert assert_never_skipped(native_lib, M, tris, pts, name) > 1000


# ---- the address checks of the call's three arrays ----
BASE = 1 << 40


def range_cases(layout):
    n = 1000
    size = [n * s for s, _ in layout]
    apart = [BASE, BASE + (1 << 30), BASE + (2 << 30)]
    out = [("apart", n, apart, OK, ())]
    for i, (s, a) in enumerate(layout):
        if not s:
            continue
        b = list(apart)
        b[i] += a // 2
        out.append(("range %d misaligned" % i, n, b, ERR_INVALID_ARG, ("range %d" % i, "aligned")))
    for i in range(3):
        for j in range(3):
            if i == j or not layout[i][0] or not layout[j][0]:
                continue
            b = list(apart)
            b[j] = b[i] + size[i]
            out.append(("range %d right behind range %d" % (j, i), n, b, OK, ()))
            b = list(apart)
            b[j] = b[i] + size[i] - layout[j][1]
            out.append(("range %d starts in the last bytes of range %d" % (j, i), n, b, ERR_INVALID_ARG, ("overlap",)))
    out.append(("2^62 records", 1 << 62, apart, ERR_INVALID_ARG, ("address space",)))
    return out


@pytest.mark.parametrize("layout", (((16, 16), (32, 16), (4, 4)), ((16, 16), (32, 16), (0, 4)), ((32, 16), (32, 16), (4, 4)), ((32, 16), (32, 16), (0, 4))),
                         ids=("points 16 B, records 32 B, instances 4 B", "the instance array left out", "32 B / 32 B / 4 B", "32 B / 32 B, left out"))
def test_query_ranges_of_the_call(native_lib, layout):
    """the call's arrays are CapPointDesc (16 B), CapClosest (32 B) and uint32 (4 B; stride 0 when left out); the 32 B / 32 B / 4 B
    layout is checked as well"""
    strides, aligns = (C.c_uint64 * 3)(*[s for s, _ in layout]), (C.c_uint32 * 3)(*[a for _, a in layout])
    table = range_cases(layout)
    assert len(table) >= 8
    for label, n, bases, code, words in table:
        if not layout[2][0]:
            bases = bases[:2] + [bases[0]]  # a left-out array is never looked at, wherever it points
        assert native_lib.cap_debug_query_ranges(n, 3, (C.c_uint64 * 3)(*bases), strides, aligns) == code, (label, native_lib.cap_last_error())
        message = native_lib.cap_last_error().decode()
        if code:
            assert all(w in message for w in words), (label, message)
