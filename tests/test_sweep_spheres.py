"""Sphere sweep queries (cap_sweep_spheres) without a GPU: the header's prototype, the export and the binding; the numpy transcription
of the contract (sweep_support.py) pinned by hand on answers that are exact in binary32, judged against its float64 twin and against a
float64 implementation by another method; the kernel's box test held to every accepted pair; the address checks of the call's two
arrays; and the model walker on the deep spirals."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import bits, needles, soup
from deep_tree_support import SIZES, depth_of, spiral, tri_boxes
from multi_hit_support import stacked_quads
from sweep_support import (MISS, RADII, contact_position_bound, degenerate, scene_magnitude, slab_times, soup_case, soup_sweeps, spiral_sweeps, sweep32,
                           sweep64, sweep_exact_pieces, sweep_queries, sweep_scene, sweep_walk, walk_start)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID_ARG = 0, 1
f32 = np.float32
FACE, EDGE_V0V1, V0 = capi.FEATURE_FACE, capi.FEATURE_EDGE_V0V1, capi.FEATURE_V0


def test_header_prototype_compiles(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "sweep.c"
    src.write_text("""#include <stddef.h>
#include "capsaicin_hip.h"
_Static_assert(sizeof(CapSweepDesc) == 32 && offsetof(CapSweepDesc, radius) == 12 && offsetof(CapSweepDesc, direction) == 16 &&
               offsetof(CapSweepDesc, tmax) == 28, "CapSweepDesc");
_Static_assert(sizeof(CapSweepHit) == 32 && offsetof(CapSweepHit, t) == 12 && offsetof(CapSweepHit, u) == 16 && offsetof(CapSweepHit, triangle) == 24 &&
               offsetof(CapSweepHit, feature) == 28, "CapSweepHit");
int (*const sweep)(CapContext*, const CapSweepDesc*, uint64_t, CapSweepHit*, const CapTraceOptions*) = cap_sweep_spheres;
""")
    subprocess.check_call([cc, "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sweep.o")])


def test_entry_point_is_exported_and_bound(native_lib):
    assert hasattr(native_lib, "cap_sweep_spheres")
    assert len(capi.SYMBOLS["cap_sweep_spheres"][1]) == 5
    assert C.sizeof(capi.SweepDesc) == 32 and C.sizeof(capi.SweepHit) == 32
    assert capi.SweepDesc.radius.offset == 12 and capi.SweepDesc.tmax.offset == 28
    assert capi.SweepHit.t.offset == 12 and capi.SweepHit.triangle.offset == 24 and capi.SweepHit.feature.offset == 28
    assert callable(capi.Renderer.sweep_spheres)
    assert native_lib.cap_sweep_spheres(None, None, 0, None, None) == ERR_INVALID_ARG
    assert b"cap_sweep_spheres: ctx is NULL" in native_lib.cap_last_error()


def test_sweep_queries_packs_the_rows():
    q = capi.Renderer.sweep_queries([(1, 2, 3), (4, 5, 6)], 0.5, [(0, 0, -1), (1, 0, 0)])
    assert q.dtype == np.float32 and q.shape == (2, 8)
    assert q[0].tolist() == [1, 2, 3, 0.5, 0, 0, -1, np.inf] and q[1].tolist() == [4, 5, 6, 0.5, 1, 0, 0, np.inf]
    q = capi.Renderer.sweep_queries([(1, 2, 3), (4, 5, 6)], [0.5, 2.0], [(0, 0, -1), (1, 0, 0)], [3.0, 4.0])
    assert q[:, 3].tolist() == [0.5, 2.0] and q[:, 7].tolist() == [3.0, 4.0]


# ---- known answers: inputs and outputs exact in binary32 ----
TRI = f32([[[0, 0, 0], [40, 0, 0], [0, 40, 0]]])
# name, origin, direction, radius, t, contact point, feature, (u, v)
KNOWN = [("face", (10, 10, 3), (0, 0, -1), 0.5, 2.5, (10, 10, 0), FACE, (0.25, 0.25)),
         ("edge", (20, -3, 10), (0, 0, -1), 5.0, 6.0, (20, 0, 0), EDGE_V0V1, (0.5, 0.0)),
         ("vertex", (-3, -4, 20), (0, 0, -1), 13.0, 8.0, (0, 0, 0), V0, (0.0, 0.0)),
         ("face from below", (10, 10, -3), (0, 0, 1), 0.5, 2.5, (10, 10, 0), FACE, (0.25, 0.25)),
         ("face, d scaled by 2", (10, 10, 3), (0, 0, -2), 0.5, 1.25, (10, 10, 0), FACE, (0.25, 0.25)),
         ("start overlap", (10, 10, 0.25), (0, 0, -1), 0.5, 0.0, (10, 10, 0), FACE, (0.25, 0.25))]


def known_sweeps():
    return np.concatenate([sweep_queries([o], r, [d]) for _, o, d, r, *_ in KNOWN])


def known_records():
    want = np.zeros((len(KNOWN), 8), f32)
    for i, (_, _, _, _, t, point, feature, uv) in enumerate(KNOWN):
        want[i, 0:3], want[i, 3], want[i, 4:6] = point, t, uv
        want.view(np.uint32)[i, 6:8] = (0, feature)
    return want


def test_known_answers_bit_for_bit():
    rec, _ = sweep_scene(known_sweeps(), TRI)
    want = known_records()
    for i, case in enumerate(KNOWN):
        assert np.array_equal(bits(rec[i]), bits(want[i])), (case[0], rec[i].tolist(), want[i].tolist())


@pytest.mark.parametrize("case", KNOWN, ids=[c[0] for c in KNOWN])
def test_known_answers_by_another_method(case):
    _, o, d, r, t, *_ = case
    got = sweep_exact_pieces(o, r, d, np.inf, TRI[0])
    assert got is not None and abs(got - t) <= 1e-9 * max(t, 1.0)


def test_tmax_at_the_contact_and_one_ulp_below():
    below = np.nextafter(f32(2.5), f32(0))
    q = sweep_queries([(10, 10, 3)] * 2, 0.5, [(0, 0, -1)] * 2, [2.5, below])
    rec, _ = sweep_scene(q, TRI)
    assert bits(rec)[0, 6] == 0 and rec[0, 3] == f32(2.5), "t <= tmax is inclusive"
    miss = np.zeros(8, f32)
    miss[3] = below
    miss.view(np.uint32)[6] = MISS
    assert np.array_equal(bits(rec[1]), bits(miss)), "the miss record carries tmax"


def test_a_sphere_passing_beside_the_triangle():
    # along y at x = -(r + margin): the nearest feature is the edge v2v0 at distance r + margin all the way
    q = sweep_queries([(-0.75, -50, 0), (-0.5, -50, 0)], 0.5, [(0, 1, 0)] * 2)
    rec, _ = sweep_scene(q, TRI)
    assert bits(rec)[0, 6] == MISS and rec[0, 3] == np.inf
    assert bits(rec)[1, 6:8].tolist() == [0, V0] and rec[1, 3] == f32(50.0), "at exactly r the path is tangent to the vertex sphere of v0"
    assert sweep_exact_pieces((-0.75, -50, 0), 0.5, (0, 1, 0), np.inf, TRI[0], span=200.0) is None


def test_direction_zero_is_a_static_overlap_test():
    q = sweep_queries([(10, 10, 0.25), (10, 10, 3)], 0.5, [(0, 0, 0)] * 2)
    rec, _ = sweep_scene(q, TRI)
    assert bits(rec)[0, 6] == 0 and rec[0, 3] == 0.0 and rec[0, 0:3].tolist() == [10, 10, 0]
    assert bits(rec)[1, 6] == MISS and rec[1, 3] == np.inf


def test_radius_zero():
    q = sweep_queries([(10, 10, 3), (-1, 10, 3), (10, 10, 0)], 0.0, [(0, 0, -1)] * 3)
    rec, _ = sweep_scene(q, TRI)
    assert bits(rec)[0, 6:8].tolist() == [0, FACE] and rec[0, 3] == f32(3.0) and rec[0, 0:3].tolist() == [10, 10, 0]
    assert bits(rec)[1, 6] == MISS
    assert bits(rec)[2, 6] == 0 and rec[2, 3] == 0.0, "a centre on the triangle is a start overlap at radius 0"


def degenerate_sweeps():
    nan, inf = np.nan, np.inf
    good = [10, 10, 3, 0.5, 0, 0, -1, inf]
    rows = []
    for col, value in ((0, nan), (1, inf), (2, -inf), (4, nan), (5, inf), (6, -inf), (3, nan), (3, -1.0), (7, nan), (7, -1.0)):
        row = list(good)
        row[col] = value
        rows.append(row)
    return f32(rows)


def test_degenerate_sweeps_give_the_miss_record_with_t_zero():
    q = degenerate_sweeps()
    assert degenerate(q).all() and not degenerate(known_sweeps()).any()
    rec, _ = sweep_scene(q, TRI)
    want = np.zeros(8, np.uint32)
    want[6] = MISS
    for i in range(len(q)):
        assert np.array_equal(bits(rec[i]), want), i
    edge = f32([[10, 10, 3, -0.0, 0, 0, -1, np.inf], [10, 10, 0.25, 0.5, 0, 0, -1, -0.0], [10, 10, 0.25, np.inf, 0, 0, -1, 0.0]])
    rec, _ = sweep_scene(edge, TRI)
    assert rec[0, 3] == f32(3.0), "radius -0 is radius 0"
    assert bits(rec)[1, 6] == 0 and rec[1, 3] == 0.0, "tmax -0 is tmax 0: the start overlap alone"
    assert bits(rec)[2, 6] == 0 and rec[2, 3] == 0.0, "radius +inf overlaps at the start"


def test_a_triangle_whose_evaluation_is_nan_is_never_the_answer():
    flat = f32([[0, 0, 0], [0, 0, 0], [0, 1, 0]])  # v0 == v1: for a point on v2's side the cascade reaches edge v0v1 with 0 / 0
    far = f32([[0, 0, -5], [1, 0, -5], [0, 1, -5]])
    q = sweep_queries([(0.1, 0.5, 2.0)], 0.25, [(0, 0, -1)])
    rec, _ = sweep_scene(q, flat[None])
    assert bits(rec)[0, 6] == MISS
    for tris, winner in ((np.stack([flat, far]), 1), (np.stack([far, flat]), 0)):
        rec, _ = sweep_scene(q, tris)
        assert bits(rec)[0, 6] == winner and rec[0, 3] == f32(6.75)


def test_stacked_quads_ties():
    n = 4
    _, tris = stacked_quads(n, 0.25)
    q = sweep_queries([(0.5, 0.5, 2.0), (0.5, 0.5, -2.0), (0.75, 0.25, 2.0)], 0.25, [(0, 0, -1), (0, 0, 1), (0, 0, -1)])
    rec, table = sweep_scene(q, tris)
    top = 2 * (n - 1)
    assert np.nonzero(table[0] == table[0].min())[0].tolist() == [top, top + 1] and bits(rec)[0, 6] == top, "the lower id of the tie"
    assert np.nonzero(table[1] == table[1].min())[0].tolist() == [0, 1] and bits(rec)[1, 6] == 0
    assert bits(rec)[2, 6] == top and rec[2, 3] == f32(1.0)
    assert rec[0, 3] == f32(1.0) and rec[1, 3] == f32(1.75)


def test_mask_restricts_the_candidates():
    _, tris = stacked_quads(4, 0.25)
    mask = np.arange(len(tris)) < 4
    q = sweep_queries([(0.75, 0.25, 2.0)], 0.25, [(0, 0, -1)])
    rec, _ = sweep_scene(q, tris, mask)
    assert bits(rec)[0, 6] == 2 and rec[0, 3] == f32(1.5)
    rec, _ = sweep_scene(sweep_queries([(0.75, 0.25, 2.0)], 0.25, [(0, 0, -1)], 1.0), tris, mask)
    assert bits(rec)[0, 6] == MISS and rec[0, 3] == f32(1.0)


# ---- the scenes of the float32 / float64 and prune tests, each made once ----
_SCENES = {}


def scene(name):
    if name not in _SCENES:
        rng = np.random.default_rng({"soup100": 31, "needles": 32, "soup4096": 33}[name])
        if name == "needles":
            tris = needles(rng, 1000)
        else:
            tris = soup(rng, 1000, edge=0.05, offset=100.0 if name == "soup100" else 4096.0)
        sweeps = np.concatenate([soup_sweeps(rng, tris, 333 if k else 334, radius) for k, radius in enumerate(RADII)])
        far = np.concatenate([soup_sweeps(rng, tris, 40, radius, far=40) for radius in RADII])
        _SCENES[name] = tris, sweeps, sweep32(sweeps, tris), far
    return _SCENES[name]


@pytest.mark.parametrize("name", ["soup100", "needles"])
def test_float32_against_float64(name):
    """The float32 function against its twin: 1 000 triangles x 1 000 sweeps, radii 0.01 to 0.1 scene sizes.

    A pair is decisive when the float64 line passes within 0.9 r of the triangle, the float64 contact lies in (0, 0.9 tmax) and the
    float64 distance at o exceeds 1.1 r.  For every decisive pair float32 must report a contact, at a time within the position error
    the prune argument claims for an accepted contact (sweep_support.contact_position_bound).

    The float64 twin's own acceptance has a knife edge at its kappa = 8 x 2^-53 (a candidate whose centre lands outside is moved in by
    the same steps), so the decisive set is taken from its first candidate time, accepted within 1e-9 r2.  Origins far from the scene
    are not in these sets: there the candidate's quadratic cancels (DESIGN.md "Sphere sweep queries", not covered)."""
    tris, sweeps, (c32, t32, *_rest), _ = scene(name)
    c64, t64, _, _, _, _, x64 = sweep64(sweeps, tris)
    r, tmax, dlen = sweeps[:, 3].astype(np.float64), sweeps[:, 7].astype(np.float64), np.linalg.norm(sweeps[:, 4:7].astype(np.float64), axis=1)
    r2 = (r * r)[:, None]
    with np.errstate(invalid="ignore"):
        hit64 = (x64["tc"] < np.inf) & (x64["dist2_c"] <= r2 * (1 + 1e-9))  # the twin's candidate, without its own knife edge
    inner = sweeps.copy()
    inner[:, 3], inner[:, 7] = (0.9 * r).astype(f32), np.inf
    x09 = sweep64(inner, tris)[6]
    r09 = inner[:, 3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        within = (x09["tc"] < np.inf) & (x09["dist2_c"] <= (r09 * r09)[:, None] * (1 + 1e-9))
        decisive = within & hit64 & (x64["tc"] > 0) & (x64["tc"] < 0.9 * tmax[:, None]) & (x64["dist2_o"] > (1.1 * r)[:, None] ** 2)
    print("%s: contacts float32 %d float64 %d, pairs that disagree %d (float64 only %d, float32 only %d)" % (
        name, c32.sum(), c64.sum(), (c32 != c64).sum(), (c64 & ~c32).sum(), (c32 & ~c64).sum()))
    both = decisive & c32
    with np.errstate(invalid="ignore"):  # (inf - inf where neither has a contact)
        err = np.abs(t32.astype(np.float64) - x64["tc"]) * dlen[:, None]
    bound = contact_position_bound(r, np.abs(sweeps[:, 0:3]).max(1), float(scene_magnitude(tris)))[:, None] * np.ones_like(err)
    print("%s: decisive pairs %d, without a float32 contact %d; largest |t32 - t64| |d| %.3g, in bounds %.3g" % (
        name, decisive.sum(), (decisive & ~c32).sum(), err[both].max(), (err[both] / bound[both]).max()))
    grazing = (c32 != c64) & ~decisive
    print("%s: grazing pairs that disagree %d" % (name, grazing.sum()))
    assert decisive.sum() > 500
    assert not (decisive & ~c32).any(), "%d of %d decisive pairs have no float32 contact" % ((decisive & ~c32).sum(), decisive.sum())
    assert np.all(err[both] <= bound[both])


def test_the_soup_holds_every_class():
    """misses, face, edge and vertex contacts and start overlaps in the GPU test's soup"""
    tris, sweeps, want = soup_case(0.0)
    ids, feat = capi.closest_triangles(want)
    for k in range(3):
        s = slice(k * len(sweeps) // 3, (k + 1) * len(sweeps) // 3)
        hit = ids[s] != MISS
        moving = hit & (want[s, 3] > 0)
        counts = [(~hit).sum(), (moving & (feat[s] == 0)).sum(), (moving & (feat[s] >= 1) & (feat[s] <= 3)).sum(), (moving & (feat[s] >= 4)).sum(),
                  (hit & (want[s, 3] == 0)).sum()]
        print("radius %g: misses %d, face %d, edge %d, vertex %d, start overlaps %d" % ((RADII[k],) + tuple(counts)))
        total = counts if k == 0 else [a + b for a, b in zip(total, counts)]
    assert min(total) > 20


# ---- the prune: the kernel's box test never rejects the box of an accepted pair ----
@pytest.mark.parametrize("name", ["soup100", "needles", "soup4096"])
def test_the_box_test_keeps_every_accepted_pair(name):
    """With the triangle's own vertex box standing for every box above it and the pair's own time for `best`: origins 1 000 scene
    sizes away and tmax = inf included."""
    tris, near, near32, far = scene(name)
    far32 = sweep32(far, tris)
    sweeps, c32, t32 = np.concatenate([near, far]), np.concatenate([near32[0], far32[0]]), np.concatenate([near32[1], far32[1]])
    mag = scene_magnitude(tris)
    i, g = np.nonzero(c32)
    assert len(i) > 1000 and (i >= len(near)).sum() > 20, "too few accepted pairs among the far origins"
    starts = [walk_start(q, mag) for q in sweeps]
    o, inv, grow = np.stack([s[0] for s in starts])[i].T, np.stack([s[1] for s in starts])[i].T, f32([s[2] for s in starts])[i]
    lo, hi = tri_boxes(tris)
    tn, ex = slab_times(o, inv, grow, lo[g].T, hi[g].T, t32[i, g])
    assert tn.dtype == np.float32 and ex.dtype == np.float32
    moving = t32[i, g] > 0
    margin = (ex.astype(np.float64) - tn)[moving] / t32[i, g][moving]
    print("%s: %d accepted pairs, %d of them from the far origins; smallest (exit - entry) / t among those with t > 0: %.3g" % (
        name, len(i), (i >= len(near)).sum(), margin.min()))
    assert np.all(tn <= ex)
    # the same boxes over [0, tmax], as the walk meets them before any contact is known
    tn, ex = slab_times(o, inv, grow, lo[g].T, hi[g].T, sweeps[i, 7])
    assert np.all(tn <= ex)


# ---- the address checks for the call's two arrays: sweeps (32 B, 16-aligned), hits (32 B, 16-aligned) ----
LAYOUT = [(32, 16), (32, 16)]
BASE = 0x7F0000010000
TOP = 1 << 64


def range_cases():
    """(label, n, bases, expected code, substrings of the message)"""
    n, out = 5, []
    apart = [BASE, BASE + n * 32 + 64]
    out.append(("aligned and disjoint", n, apart, OK, ()))
    for i in range(2):
        for off in (4, 8, 12):
            b = list(apart)
            b[i] += off
            out.append(("range %d misaligned by %d" % (i, off), n, b, ERR_INVALID_ARG, ("range %d" % i, "16-byte aligned")))
    out.append(("hits right behind the sweeps", n + 1, [BASE, BASE + (n + 1) * 32], OK, ()))
    out.append(("sweeps right behind the hits", n + 1, [BASE + (n + 1) * 32, BASE], OK, ()))
    out.append(("hits start in the last sweep", n, [BASE, BASE + (n - 1) * 32 + 16], ERR_INVALID_ARG, ("range 0", "range 1", "overlap")))
    out.append(("sweeps start in the last hit", n, [BASE + (n - 1) * 32 + 16, BASE], ERR_INVALID_ARG, ("range 0", "range 1", "overlap")))
    out.append(("in place", n, [BASE, BASE], ERR_INVALID_ARG, ("overlap",)))
    out.append(("2^61 sweeps", 1 << 61, apart, ERR_INVALID_ARG, ("range 0", "address space")))
    for i, (stride, align) in enumerate(LAYOUT):
        fits = (TOP - 1 - n * stride) // align * align
        for b_i, code in ((fits, OK), (fits + align, ERR_INVALID_ARG)):
            b = list(apart)
            b[i] = b_i
            out.append(("range %d at 2^64 - %d" % (i, TOP - b_i), n, b, code, ("range %d" % i, "address space") if code else ()))
    return out


def test_query_ranges_of_the_call(native_lib):
    strides, aligns = (C.c_uint64 * 2)(*[s for s, _ in LAYOUT]), (C.c_uint32 * 2)(*[a for _, a in LAYOUT])
    table = range_cases()
    assert len(table) > 12
    for label, n, bases, code, words in table:
        assert native_lib.cap_debug_query_ranges(n, 2, (C.c_uint64 * 2)(*bases), strides, aligns) == code, (label, native_lib.cap_last_error())
        message = native_lib.cap_last_error().decode()
        if code:
            assert all(w in message for w in words), (label, message)


# ---- the deep spirals: the model walk fills the stack of every class ----
@pytest.mark.parametrize("n", SIZES)
def test_sweeps_fill_the_stack(native_lib, n):
    """depth - 1 entries at once (depth - 2 for n = 40, as for rays and points), so a walk compiled with the class below would drop a
    push; and the model's winners are the brute force's."""
    tris = spiral(n)
    nodes, order, depth = capi.host_sah_build(*tri_boxes(tris))
    assert depth == depth_of(n)
    sweeps = spiral_sweeps(n)
    want, table = sweep_scene(sweeps, tris)
    res = [sweep_walk(nodes, order, tris, q, table[i]) for i, q in enumerate(sweeps) if not degenerate(q)[0]]
    high = max(h for h, _, _, _ in res)
    print("spiral n %d: depth %d, model high-water %d" % (n, depth, high))
    assert depth - (2 if n == 40 else 1) <= high <= depth
    assert any(g is not None and slot == high - 1 for _, g, slot, _ in res), "no answer comes out of the highest slot used"
    ids = capi.closest_triangles(want)[0][~degenerate(sweeps)]
    assert [MISS if g is None else g for _, g, _, _ in res] == ids.tolist()
    assert (ids == MISS).any() and (ids != MISS).sum() > len(ids) // 2
