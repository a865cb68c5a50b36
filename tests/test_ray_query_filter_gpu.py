"""Ray flags and instance masks of the ray queries (cap_trace_rays_ex, cap_trace_occlusion_ex, cap_trace_rays_multi_ex,
cap_scene_set_instance_masks) on the MI355X.  Every comparison is equality of raw bits and no ray is left out: against the brute
force of filter_support (the oracle's triangle test filtered by the contract's own facing sign and the mesh masks) on stacked quads
with one mesh per quad and both windings, the Cornell box and the 262 k hall (float64 candidate supersets), across the wide and
binary kernels and every builder; a partition property on a million rays that needs no helper; the plain calls' bytes through the
new entry points; first-hit membership; far and degenerate rays; the launch split; the state and argument contract; and a render
that filtered queries and mask changes leave untouched."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from filter_support import (MISS, bits, closest_record, faced_hits, filtered_hits, filtered_occlusion, mesh_of_triangles,
                            stacked_quads_meshes)
from multi_hit_support import candidate_superset, expected_pages, hit_list_array
from refit_support import context, hall_camera, hall_scene, Scene
from test_ray_query_multi_gpu import STAT_COUNTERS, degenerate_rays, hall_rays, ray_array

pytestmark = pytest.mark.gpu
BUILDERS = (0, 1, 2, 3, 4)
CULLS = (None, "back", "front")
ERR_INVALID_ARG, ERR_STATE = 1, 3
SENTINEL = 0x7FBADBAD
FIRST, BACK, FRONT = 0x04, 0x10, 0x20


def options(flags=0, mask=0, r0=0, r1=0):
    o = capi.TraceOptions(flags, mask)
    o.reserved[0], o.reserved[1] = r0, r1
    return o


def ref(o):
    return None if o is None else ctypes.byref(o)


def raw_closest(r, rays_t, o):
    import torch
    out = torch.empty((len(rays_t), 4), dtype=torch.float32, device=rays_t.device)
    torch.cuda.synchronize()
    assert capi.lib().cap_trace_rays_ex(r.ctx, rays_t.data_ptr(), len(rays_t), out.data_ptr(), ref(o)) == 0, capi.lib().cap_last_error()
    r.sync()
    return bits(out.cpu().numpy())


def raw_occlusion(r, rays_t, o):
    import torch
    out = torch.empty((len(rays_t),), dtype=torch.int32, device=rays_t.device)
    torch.cuda.synchronize()
    assert capi.lib().cap_trace_occlusion_ex(r.ctx, rays_t.data_ptr(), len(rays_t), out.data_ptr(), ref(o)) == 0, capi.lib().cap_last_error()
    r.sync()
    return out.cpu().numpy()


def raw_multi(r, rays_t, k, o, page=None):
    import torch
    n = len(rays_t)
    hits = torch.empty((n, k, 4), dtype=torch.float32, device=rays_t.device) if page is None else page
    cnt = torch.empty((n,), dtype=torch.int32, device=rays_t.device)
    torch.cuda.synchronize()
    assert capi.lib().cap_trace_rays_multi_ex(r.ctx, rays_t.data_ptr(), n, k, hits.data_ptr(), cnt.data_ptr(), 0 if page is None else 1,
                                              ref(o)) == 0, capi.lib().cap_last_error()
    r.sync()
    return bits(hits.cpu().numpy()), cnt.cpu().numpy()


def page_out(r, rays, k, cull, mask, limit=200):
    """pages of k records under the filter until every page is empty: the per-ray concatenation of the records before the first miss"""
    page = r.trace_rays_multi(rays, k, cull=cull, mask=mask)
    pages = [page.copy()]
    for _ in range(limit):
        if np.all(bits(page)[:, 0, 3] == MISS):
            break
        page = r.trace_rays_multi(rays, k, resume=page, cull=cull, mask=mask)
        pages.append(page.copy())
    else:
        raise AssertionError("paging did not end")
    out = []
    for i in range(len(rays)):
        recs = np.concatenate([p[i] for p in pages])
        out.append(recs[bits(recs)[:, 3] != MISS])
    return out


def check_filtered(r, rays, lists, occ, cull, mask, ks=(1, 4, 16), paging=(), what=""):
    """closest, occlusion, pages, counts and paging of one (cull, mask) against the filtered brute force `lists` / `occ`"""
    want1 = np.stack([closest_record(h, x[7]) for x, h in zip(rays, lists)])
    got = r.trace_rays(rays, cull=cull, mask=mask)
    bad = np.nonzero((bits(got) != bits(want1)).any(1))[0]
    assert len(bad) == 0, "%s closest: %d rays differ, first %d: got %s want %s" % (what, len(bad), bad[0], bits(got[bad[0]]), bits(want1[bad[0]]))
    if occ is not None:
        got = r.trace_occlusion(rays, cull=cull, mask=mask)
        bad = np.nonzero(got != occ)[0]
        assert len(bad) == 0, "%s occlusion: %d rays differ, first %d" % (what, len(bad), bad[0])
    for k in ks:
        want, cnt = expected_pages(rays, lists, k)
        got = r.trace_rays_multi(rays, k, cull=cull, mask=mask)
        bad = np.nonzero((bits(got) != bits(want)).any((1, 2)))[0]
        assert len(bad) == 0, "%s k=%d: %d rays differ, first %d" % (what, k, len(bad), bad[0])
        got, c = r.trace_rays_multi(rays, k, counts=True, cull=cull, mask=mask)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(c, cnt), "%s k=%d with counts" % (what, k)
    _, c = r.trace_rays_multi(rays, 0, counts=True, cull=cull, mask=mask)
    assert np.array_equal(c, np.array([len(h) for h in lists], np.int32)), "%s counts only" % what
    for k in paging:
        walked = page_out(r, rays, k, cull, mask)
        for i in range(len(rays)):
            assert np.array_equal(bits(walked[i]), bits(hit_list_array(lists[i]))), "%s paging k=%d ray %d" % (what, k, i)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. stacked quads, one mesh per quad, every third quad wound the other way
QUAD_MASKS = {  # name -> (mask table or None, inclusion mask or None)
    "all": (None, None),
    "every other quad": (np.where(np.arange(40) % 2 == 0, 0x01, 0x02).astype(np.uint8), 0x01),
    "one quad": (np.where(np.arange(40) == 7, 0x80, 0x40).astype(np.uint8), 0x80),
    "nothing": (np.where(np.arange(40) % 2 == 0, 0x01, 0x02).astype(np.uint8), 0x04),
}


@pytest.fixture(scope="module")
def quads():
    arrays, tris = stacked_quads_meshes(40, 0.25, flip_every=3)
    mot = mesh_of_triangles(arrays[4])
    rng = np.random.default_rng(17)
    n = 40
    sets = []
    xy = rng.uniform(0.02, 0.98, (n, 2))
    sets.append(ray_array(np.c_[xy, np.full(n, -0.5)], 0.0, np.tile([0, 0, 1.0], (n, 1)), np.inf))  # through every quad, upwards
    sets.append(ray_array(np.c_[xy, np.full(n, 10.5)], 0.0, np.tile([0, 0, -1.0], (n, 1)), np.inf))  # and downwards
    s = rng.uniform(0.05, 0.95, n).astype(np.float32)  # on the shared diagonal: equal-t pairs
    sets.append(ray_array(np.c_[s, s, np.full(n, 10.5)], 0.0, np.tile([0, 0, -1.0], (n, 1)), np.inf))
    zs = (rng.integers(0, 39, n) * 0.25 + 0.125).astype(np.float32)  # between quads, both directions, cut intervals
    sets.append(ray_array(np.c_[rng.uniform(0.02, 0.98, (n, 2)), zs], rng.uniform(0, 0.5, n), np.c_[np.zeros((n, 2)), rng.choice([-1.0, 1.0], n)],
                          rng.uniform(0.5, 4.0, n)))
    o = np.c_[rng.uniform(-0.5, 1.5, (n, 2)), rng.uniform(-1, 11, n)]  # slanted, from anywhere
    sets.append(ray_array(o, 0.0, np.c_[rng.normal(size=(n, 2)) * 0.1, rng.choice([-1.0, 1.0], n)], np.inf))
    rays = np.concatenate(sets).astype(np.float32)
    faced = [faced_hits(x, tris) for x in rays]
    # the cases the filters must not get wrong: equal-t pairs, and rays whose nearest unfiltered hit is rejected by each filter
    assert sum(1 for h in faced for a, b in zip(h, h[1:]) if a[0] == b[0]) > 100
    expect = {}
    for cull in CULLS:
        for name, (masks, mask) in QUAD_MASKS.items():
            lists = [filtered_hits(x, tris, mot, masks, cull, mask, faced=f) for x, f in zip(rays, faced)]
            occ = np.array([filtered_occlusion(x, tris, mot, masks, cull, mask) for x in rays], np.int32)
            expect[cull, name] = (lists, occ)
            if name != "nothing" and (cull is not None or name != "all"):
                culled_first = sum(1 for f, h in zip(faced, lists) if h and f[0][3] != h[0][3])
                assert culled_first > 20, (cull, name, culled_first)
    assert all(len(h) == 0 for h in expect[None, "nothing"][0]) and max(len(h) for h in expect["back", "all"][0]) > 16
    return Scene(*arrays), tris, mot, rays, faced, expect


@pytest.mark.parametrize("build", BUILDERS)
def test_stacked_quads_brute_force(native_lib, quads, build):
    scene, tris, mot, rays, faced, expect = quads
    r = context(scene, build)
    try:
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            assert r.debug_get(capi.Renderer.DEBUG_WIDE_IN_USE) == 1 - no_wide
            for name, (masks, mask) in QUAD_MASKS.items():
                r.set_instance_masks(masks)
                for cull in CULLS:
                    lists, occ = expect[cull, name]
                    check_filtered(r, rays, lists, occ, cull, mask, paging=(1, 4, 16),
                                   what="builder %d no_wide8 %d cull %s masks %s" % (build, no_wide, cull, name))
    finally:
        r.close()


# 2. Cornell box (8 meshes) and the 262 k hall (12 meshes): per-mesh masks with distinct bits
def mesh_bits(n):
    return (1 << (np.arange(n) % 8)).astype(np.uint8)


@pytest.fixture(scope="module")
def cornell(cornell_path):
    from refit_support import cornell_scene
    scene, _ = cornell_scene(cornell_path)
    assert len(scene.meshes) == 8
    tris = scene.triangles()
    rng = np.random.default_rng(6)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    c = (lo + hi) / 2

    def dirs(n):
        v = rng.normal(size=(n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    sets = [ray_array(rng.uniform(lo + 0.02, hi - 0.02, (1500, 3)), 0.0, dirs(1500), np.where(rng.random(1500) < 0.5, np.inf, 100.0))]
    for radius, n in ((4.0, 500), (60.0, 200)):  # outside; 60: beyond the wide view's budget, handed to the binary kernel
        o = c + dirs(n) * radius
        sets.append(ray_array(o, 0.0, rng.uniform(lo, hi, (n, 3)) - o, np.inf))
    pts = np.concatenate([tris.reshape(-1, 3), (tris[:, 0] + tris[:, 1]) / 2, (tris[:, 1] + tris[:, 2]) / 2, (tris[:, 0] + tris[:, 2]) / 2])
    for _ in range(3):  # at shared edges and vertices
        o = rng.uniform(lo + 0.05, hi - 0.05, (len(pts), 3)).astype(np.float32)
        sets.append(ray_array(o, 0.0, pts - o, np.inf))
    k = rng.integers(0, len(tris), 500)  # from surfaces
    b = rng.dirichlet((1, 1, 1), 500).astype(np.float32)
    o = (tris[k] * b[:, :, None]).sum(1).astype(np.float32)
    for tmin in (0.0, 1e-4):
        sets.append(ray_array(o, tmin, dirs(500), np.inf))
    rays = np.concatenate(sets).astype(np.float32)
    assert len(rays) >= 3500
    return scene, tris, rays, [faced_hits(x, tris) for x in rays]


def test_cornell_brute_force(native_lib, cornell):
    scene, tris, rays, faced = cornell
    mot = mesh_of_triangles(scene.meshes)
    masks = mesh_bits(8)
    r = context(scene)
    try:
        r.set_instance_masks(masks)
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            for cull in CULLS:
                for mask in (0x08, 0x55, 0xFF):  # one mesh, half of them, all
                    lists = [filtered_hits(x, tris, mot, masks, cull, mask, faced=f) for x, f in zip(rays, faced)]
                    occ = None
                    if no_wide == 0 or mask == 0x55:
                        occ = np.array([filtered_occlusion(x, tris, mot, masks, cull, mask) for x in rays], np.int32)
                    check_filtered(r, rays, lists, occ, cull, mask, ks=(1, 4, 16) if no_wide == 0 else (4,),
                                   what="cornell no_wide8 %d cull %s mask 0x%x" % (no_wide, cull, mask))
    finally:
        r.close()


@pytest.fixture(scope="module")
def hall():
    s = hall_scene(1.0)
    assert len(s.indices) // 3 > 250000 and len(s.meshes) == 12
    return s, s.triangles()


def test_hall_against_candidates(native_lib, hall):
    scene, tris = hall
    mot = mesh_of_triangles(scene.meshes)
    masks = mesh_bits(12)
    rays = hall_rays(tris, np.random.default_rng(19))
    cands = candidate_superset(rays, tris)
    r = context(scene)
    try:
        assert r.debug_get(capi.Renderer.DEBUG_WIDE_IN_USE) == 1
        # every triangle a page names joins the candidates, so a record outside the float64 superset cannot pass unseen
        named = [set() for _ in rays]
        for cull in CULLS:
            page = r.trace_rays_multi(rays, 16, cull=cull)
            for i in range(len(rays)):
                named[i] |= {int(g) for g in bits(page[i])[:, 3] if g != MISS}
        faced = [faced_hits(rays[i], tris, cands[i] + sorted(named[i])) for i in range(len(rays))]
        r.set_instance_masks(masks)
        seen = set()
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            for cull in CULLS:
                for mask in (0x40, 0x0F, 0xFF):  # one mesh (6, the largest), half of them, all
                    lists = [filtered_hits(x, tris, mot, masks, cull, mask, faced=f) for x, f in zip(rays, faced)]
                    occ = np.array([filtered_occlusion(rays[i], tris, mot, masks, cull, mask, cands=cands[i] + sorted(named[i]))
                                    for i in range(len(rays))], np.int32)
                    check_filtered(r, rays, lists, occ, cull, mask, ks=(1, 16) if no_wide == 0 else (4,), paging=(16,) if mask == 0xFF else (),
                                   what="hall no_wide8 %d cull %s mask 0x%x" % (no_wide, cull, mask))
                    seen.add((cull, mask, sum(len(h) for h in lists) > 0))
        assert all(s[2] for s in seen)  # every combination has hits to get right
        ref_pages = {(cull, mask): r.trace_rays_multi(rays, 16, counts=True, cull=cull, mask=mask) for cull in CULLS for mask in (0x40, 0x0F)}
    finally:
        r.close()
    for build in (1, 2, 3, 4):  # every builder gives the same bits (the binary kernels made ref_pages)
        rb = context(scene, build)
        try:
            rb.set_instance_masks(masks)
            for (cull, mask), (p0, c0) in ref_pages.items():
                p, c = rb.trace_rays_multi(rays, 16, counts=True, cull=cull, mask=mask)
                assert np.array_equal(bits(p), bits(p0)) and np.array_equal(c, c0), "builder %d cull %s mask 0x%x" % (build, cull, mask)
        finally:
            rb.close()


# 3. a partition property that needs no helper: front- and back-facing hits partition a ray's hits
def test_cull_partition_on_a_million_rays(native_lib, hall):
    import torch
    scene, tris = hall
    dev = torch.device("cuda", 0)
    n = 1 << 20
    g = torch.Generator(device=dev)
    g.manual_seed(23)
    lo = torch.as_tensor(tris.reshape(-1, 3).min(0), device=dev)
    hi = torch.as_tensor(tris.reshape(-1, 3).max(0), device=dev)
    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = lo + (hi - lo) * torch.rand((n, 3), generator=g, device=dev)
    d = torch.randn((n, 3), generator=g, device=dev)
    rays[:, 4:7] = d / d.norm(dim=1, keepdim=True)
    rays[:, 7] = float("inf")
    r = context(scene)
    try:
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            cnt = {c: r.trace_rays_multi(rays, 0, counts=True, cull=c)[1] for c in CULLS}
            assert torch.equal(cnt["back"] + cnt["front"], cnt[None]) and int(cnt[None].sum()) > n // 2
            assert int((cnt["back"] > 0).sum()) > 1000 and int((cnt["front"] > 0).sum()) > 1000  # both facings occur
            plain = r.trace_rays(rays).view(torch.int32)
            a, b = r.trace_rays(rays, cull="back"), r.trace_rays(rays, cull="front")
            ai, bi = a.view(torch.int32), b.view(torch.int32)
            # (t, id) minimum of the two culled records; ids as unsigned (a miss is 0xFFFFFFFF, above every id)
            ida, idb = ai[:, 3].to(torch.int64) & 0xFFFFFFFF, bi[:, 3].to(torch.int64) & 0xFFFFFFFF
            take_a = (a[:, 0] < b[:, 0]) | ((a[:, 0] == b[:, 0]) & (ida <= idb))
            assert torch.equal(torch.where(take_a[:, None], ai, bi), plain), "no_wide8 %d" % no_wide
            # and the culled closest hit exists exactly where the culled count is not zero
            assert torch.equal(ida != MISS, cnt["back"] > 0) and torch.equal(idb != MISS, cnt["front"] > 0)
    finally:
        r.close()


# 4. the plain calls through the new entry points
def test_null_and_zero_options_are_the_plain_calls(native_lib, hall, cornell):
    import torch
    dev = torch.device("cuda", 0)
    for scene, rays in ((hall[0], hall_rays(hall[1], np.random.default_rng(29))), (cornell[0], cornell[2])):
        t = torch.as_tensor(rays, device=dev)
        r = context(scene)
        try:
            for no_wide in (0, 1):
                r.debug_switch("CAP_NO_WIDE8", no_wide)
                plain = (bits(r.trace_rays(rays)), r.trace_occlusion(rays)) + tuple(
                    x if x.dtype != np.float32 else bits(x) for x in r.trace_rays_multi(rays, 16, counts=True))

                def same(o, what):
                    p, c = raw_multi(r, t, 16, o)
                    assert np.array_equal(raw_closest(r, t, o), plain[0]) and np.array_equal(raw_occlusion(r, t, o), plain[1]), what
                    assert np.array_equal(p, plain[2]) and np.array_equal(c, plain[3]), what

                same(None, "NULL options")
                same(options(), "zero options")
                for m in (0x01, 0x80, 0xFF):  # no table installed: every mask is 0xFF and passes any inclusion mask
                    same(options(0, m), "inclusion mask 0x%x without a table" % m)
                r.set_instance_masks(np.full(len(scene.meshes), 0xFF, np.uint8))
                same(options(0, 0x10), "all-0xFF masks")
                r.set_instance_masks(np.full(len(scene.meshes), 0x0F, np.uint8))  # a table that passes everything: the filtered kernels
                same(options(0, 0x01), "masks 0x0F, inclusion 0x01")
                same(None, "masks 0x0F, plain call")
                assert np.array_equal(bits(r.trace_rays_multi(rays, 16, mask=0x10)[:, :, 3]), np.full((len(rays), 16), MISS, np.uint32))
                r.set_instance_masks(None)
                same(options(0, 0x10), "masks restored")
        finally:
            r.close()


# 5. first hit: some member of the filtered set, a miss exactly where the closest query misses
def test_first_hit_is_a_member(native_lib, quads, cornell):
    qs, qtris, qmot, qrays, qfaced, _ = quads
    cs, ctris, crays, cfaced = cornell
    qmasks = QUAD_MASKS["every other quad"][0]
    for scene, tris, rays, faced, masks, mask in ((qs, qtris, qrays, qfaced, qmasks, 0x01), (cs, ctris, crays, cfaced, mesh_bits(8), 0x55)):
        mot = mesh_of_triangles(scene.meshes)
        for build in (0, 2):
            r = context(scene, build)
            try:
                for no_wide in (0, 1):
                    r.debug_switch("CAP_NO_WIDE8", no_wide)
                    for table, m in ((None, None), (masks, mask)):
                        r.set_instance_masks(table)
                        for cull in CULLS:
                            got = r.trace_rays(rays, cull=cull, mask=m, first_hit=True)
                            closest = r.trace_rays(rays, cull=cull, mask=m)
                            assert np.array_equal(bits(got)[:, 3] == MISS, bits(closest)[:, 3] == MISS)
                            n_other = 0
                            for i, x in enumerate(rays):
                                members = filtered_hits(x, tris, mot, table, cull, m, faced=faced[i])
                                if not members:
                                    assert np.array_equal(bits(got[i]), bits(closest_record([], x[7]))), i
                                    continue
                                recs = bits(hit_list_array(members))
                                assert (recs == bits(got[i])).all(1).any(), "ray %d: %s is not among its %d hits" % (i, bits(got[i]), len(members))
                                n_other += int(not np.array_equal(bits(got[i]), bits(closest[i])))
                            # occlusion accepts the flag and answers as without it
                            import torch
                            t = torch.as_tensor(rays, device=torch.device("cuda", 0))
                            fl = {None: 0, "back": BACK, "front": FRONT}[cull]
                            assert np.array_equal(raw_occlusion(r, t, options(fl | FIRST, m or 0)), raw_occlusion(r, t, options(fl, m or 0)))
            finally:
                r.close()


# 6. far origins, degenerate rays and the launch split under filters
def test_far_and_degenerate_rays(native_lib, quads):
    scene, tris, mot, rays, faced, expect = quads
    far = rays[:80].copy()  # the vertical rays from 1e4 scene sizes away: handed to the binary kernel by the wide one
    far[:40, 2], far[40:, 2] = -1.0e5, 1.0e5
    masks, mask = QUAD_MASKS["every other quad"]
    deg = degenerate_rays()
    r = context(scene)
    try:
        r.set_instance_masks(masks)
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            for cull in CULLS:
                lists = [filtered_hits(x, tris, mot, masks, cull, mask) for x in far]
                occ = np.array([filtered_occlusion(x, tris, mot, masks, cull, mask) for x in far], np.int32)
                check_filtered(r, far, lists, occ, cull, mask, ks=(1, 16), paging=(4,), what="far no_wide8 %d cull %s" % (no_wide, cull))
                first = r.trace_rays(far, cull=cull, mask=mask, first_hit=True)
                for i in range(len(far)):
                    recs = bits(hit_list_array(lists[i])) if lists[i] else bits(closest_record([], far[i, 7]))[None]
                    assert (recs == bits(first[i])).all(1).any(), i
                # degenerate rays: miss records, occlusion 0, count 0, whatever the filter
                want = np.zeros((len(deg), 4), np.float32)
                want[:, 0] = deg[:, 7]
                want.view(np.uint32)[:, 3] = MISS
                for fh in (False, True):
                    assert np.array_equal(bits(r.trace_rays(deg, cull=cull, mask=mask, first_hit=fh)), bits(want))
                assert np.all(r.trace_occlusion(deg, cull=cull, mask=mask) == 0)
                p, c = r.trace_rays_multi(deg, 3, counts=True, cull=cull, mask=mask)
                assert np.array_equal(bits(p), bits(np.repeat(want[:, None], 3, 1))) and np.all(c == 0)
    finally:
        r.close()


def test_launch_split_with_a_filter(native_lib, quads):
    import torch
    scene, tris, mot, rays, faced, expect = quads
    dev = torch.device("cuda", 0)
    n = (1 << 24) + 5
    masks, mask = QUAD_MASKS["every other quad"]
    lists, occ = expect["front", "every other quad"]
    reps = (n + len(rays) - 1) // len(rays)
    r = context(scene)
    try:
        r.set_instance_masks(masks)
        t = torch.as_tensor(rays, device=dev).repeat(reps, 1)[:n].contiguous()
        o = options(FRONT, mask)
        buf = torch.full((n + 4, 4), SENTINEL, dtype=torch.int32, device=dev)
        assert capi.lib().cap_trace_rays_ex(r.ctx, t.data_ptr(), n, buf.data_ptr(), ctypes.byref(o)) == 0
        r.sync()
        want = torch.as_tensor(bits(np.stack([closest_record(h, x[7]) for x, h in zip(rays, lists)])).view(np.int32), device=dev)
        assert torch.equal(buf[:n], want.repeat(reps, 1)[:n]) and bool((buf[n:] == SENTINEL).all())
        occ_buf = torch.full((n + 4,), SENTINEL, dtype=torch.int32, device=dev)
        assert capi.lib().cap_trace_occlusion_ex(r.ctx, t.data_ptr(), n, occ_buf.data_ptr(), ctypes.byref(o)) == 0
        cnt = torch.full((n + 4,), SENTINEL, dtype=torch.int32, device=dev)
        assert capi.lib().cap_trace_rays_multi_ex(r.ctx, t.data_ptr(), n, 0, None, cnt.data_ptr(), 0, ctypes.byref(o)) == 0
        r.sync()
        assert torch.equal(occ_buf[:n], torch.as_tensor(occ, device=dev).repeat(reps)[:n]) and bool((occ_buf[n:] == SENTINEL).all())
        wc = torch.as_tensor(np.array([len(h) for h in lists], np.int32), device=dev).repeat(reps)[:n]
        assert torch.equal(cnt[:n], wc) and bool((cnt[n:] == SENTINEL).all())
    finally:
        r.close()


# 7. the state and argument contract
def test_argument_and_state_contract(native_lib, quads):
    import torch
    scene, tris, mot, qrays, faced, expect = quads
    dev = torch.device("cuda", 0)
    L = capi.lib()
    rays = torch.as_tensor(qrays[:128], device=dev).contiguous()
    hits = torch.full((128 * 16 + 8, 4), SENTINEL, dtype=torch.int32, device=dev)
    occ = torch.full((136,), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((136,), SENTINEL, dtype=torch.int32, device=dev)
    R, H, O_, C = rays.data_ptr(), hits.data_ptr(), occ.data_ptr(), cnt.data_ptr()
    ok = options(BACK, 0x01)
    m40 = np.full(40, 0x01, np.uint8)
    r = capi.Renderer(0)
    try:
        closest = lambda o, rp=R, n=128, hp=H: L.cap_trace_rays_ex(r.ctx, rp, n, hp, ref(o))
        any_ = lambda o, rp=R, n=128, op=O_: L.cap_trace_occlusion_ex(r.ctx, rp, n, op, ref(o))
        multi = lambda o, k=4, fl=0, rp=R, n=128, hp=H, cp=C: L.cap_trace_rays_multi_ex(r.ctx, rp, n, k, hp, cp, fl, ref(o))
        assert L.cap_scene_set_instance_masks(r.ctx, m40.ctypes.data, 40) == ERR_STATE  # before cap_scene_upload
        assert L.cap_scene_set_instance_masks(None, m40.ctypes.data, 40) == ERR_INVALID_ARG
        r.upload_scene(scene.positions, scene.normals, scene.texcoords, scene.indices, scene.meshes)
        assert L.cap_scene_set_instance_masks(r.ctx, m40.ctypes.data, 39) == ERR_INVALID_ARG  # not the scene's mesh count
        assert L.cap_scene_set_instance_masks(r.ctx, None, 41) == ERR_INVALID_ARG
        assert L.cap_scene_set_instance_masks(r.ctx, m40.ctypes.data, 40) == 0  # allowed before the build
        assert L.cap_scene_set_instance_masks(r.ctx, None, 40) == 0
        for f in (closest, any_, multi):
            assert f(ok) == ERR_STATE and f(None) == ERR_STATE  # before cap_bvh_build
        r.build_bvh()
        for f in (closest, any_, multi):
            assert f(options(BACK | FRONT)) == ERR_INVALID_ARG  # both culls
            for bad in (0x01, 0x02, 0x08, 0x40, 0x100, 0x80000000):
                assert f(options(bad)) == ERR_INVALID_ARG and f(options(bad | BACK)) == ERR_INVALID_ARG  # unknown bits
            assert f(options(BACK, 0, 1, 0)) == ERR_INVALID_ARG and f(options(0, 0, 0, 7)) == ERR_INVALID_ARG  # reserved
            assert f(options(0, 0x100)) == ERR_INVALID_ARG and f(options(BACK, 0xFFFFFFFF)) == ERR_INVALID_ARG  # mask beyond 8 bits
        assert multi(options(FIRST)) == ERR_INVALID_ARG and multi(options(FIRST | BACK, 1)) == ERR_INVALID_ARG  # no first hit in a multi query
        # everything else as for the plain calls
        assert closest(ok, None) == ERR_INVALID_ARG and closest(ok, R, 128, None) == ERR_INVALID_ARG and any_(ok, R, 128, None) == ERR_INVALID_ARG
        assert closest(ok, R + 4, 64) == ERR_INVALID_ARG and closest(ok, R, 64, H + 8) == ERR_INVALID_ARG and any_(ok, R + 4, 64) == ERR_INVALID_ARG
        assert closest(ok, R, 128, R + 32 * 64) == ERR_INVALID_ARG and any_(ok, R, 128, R + 32 * 127) == ERR_INVALID_ARG  # overlap
        assert multi(ok, 17) == ERR_INVALID_ARG and multi(ok, 0) == ERR_INVALID_ARG and multi(ok, 4, 2) == ERR_INVALID_ARG
        assert multi(ok, 4, 0, R, 128, H, R + 32 * 127) == ERR_INVALID_ARG and multi(ok, 16, 0, R, 1 << 58, H, None) == ERR_INVALID_ARG
        assert closest(ok, R, 1 << 61) == ERR_INVALID_ARG
        assert L.cap_trace_rays_ex(None, R, 1, H, ref(ok)) == ERR_INVALID_ARG and L.cap_trace_occlusion_ex(None, R, 1, O_, ref(ok)) == ERR_INVALID_ARG
        assert L.cap_trace_rays_multi_ex(None, R, 1, 1, H, C, 0, ref(ok)) == ERR_INVALID_ARG
        assert closest(ok, R, 0) == 0 and any_(ok, R, 0) == 0 and multi(ok, 4, 0, R, 0) == 0  # nothing to do
        r.sync()
        torch.cuda.synchronize()
        assert bool((hits == SENTINEL).all()) and bool((occ == SENTINEL).all()) and bool((cnt == SENTINEL).all())  # nothing was written
        # the binding's own checks
        with pytest.raises(capi.CapError):
            r.trace_rays(rays, cull="both")
        with pytest.raises(capi.CapError):
            r.trace_rays(rays, mask=0x100)
        with pytest.raises(capi.CapError):
            r.set_instance_masks(np.zeros(39, np.uint8))

        # masks survive a rebuild with another builder, a vertex update + refit; an upload resets them
        masks, mask = QUAD_MASKS["every other quad"]
        lists = expect["front", "every other quad"][0]
        want = bits(np.stack([closest_record(h, x[7]) for x, h in zip(qrays, lists)]))
        unmasked = bits(np.stack([closest_record(h, x[7]) for x, h in zip(qrays, expect["front", "all"][0])]))
        assert not np.array_equal(want, unmasked)
        r.set_instance_masks(masks)
        assert np.array_equal(bits(r.trace_rays(qrays, cull="front", mask=mask)), want)
        for build in (2, 1):
            r.set_bvh_build(build)
            r.build_bvh()
            assert np.array_equal(bits(r.trace_rays(qrays, cull="front", mask=mask)), want), "after cap_bvh_build %d" % build
        r.update_vertices(positions=scene.positions)
        assert closest(ok) == ERR_STATE and any_(ok) == ERR_STATE and multi(ok) == ERR_STATE  # stale trees
        assert L.cap_scene_set_instance_masks(r.ctx, masks.ctypes.data, 40) == 0  # does not need fresh trees, and does not refresh them
        assert closest(ok) == ERR_STATE
        r.refit_bvh()
        assert np.array_equal(bits(r.trace_rays(qrays, cull="front", mask=mask)), want), "after refit"
        r.upload_scene(scene.positions, scene.normals, scene.texcoords, scene.indices, scene.meshes)
        r.build_bvh()
        assert np.array_equal(bits(r.trace_rays(qrays, cull="front", mask=mask)), unmasked), "cap_scene_upload resets the masks"

        # a mask change between two enqueued queries takes effect for the second only; host bytes may go when the call returns
        big = torch.as_tensor(qrays, device=dev).repeat(2000, 1).contiguous()
        o = options(FRONT, mask)
        out1, out2 = torch.empty((len(big), 4), device=dev), torch.empty((len(big), 4), device=dev)
        torch.cuda.synchronize()
        assert L.cap_trace_rays_ex(r.ctx, big.data_ptr(), len(big), out1.data_ptr(), ref(o)) == 0
        tmp = masks.copy()
        assert L.cap_scene_set_instance_masks(r.ctx, tmp.ctypes.data, 40) == 0
        tmp[:] = 0
        assert L.cap_trace_rays_ex(r.ctx, big.data_ptr(), len(big), out2.data_ptr(), ref(o)) == 0
        assert L.cap_scene_set_instance_masks(r.ctx, None, 40) == 0
        r.sync()
        assert np.array_equal(bits(out1.cpu().numpy()), np.tile(unmasked, (2000, 1))) and np.array_equal(bits(out2.cpu().numpy()), np.tile(want, (2000, 1)))
    finally:
        r.close()


# 8. a render interrupted by filtered queries and mask changes is unchanged
def test_filters_do_not_interfere_with_rendering(native_lib, bluenoise, hall):
    """Frames 0-3 on two batch lanes, masks set and filtered queries enqueued behind them while they run (device rays, no host sync
    of the queries), frames 4-7 into the same accumulation with the masks still installed: accumulation, post output, AOV planes
    and every CapStats counter equal a run without them (cap_render ignores the masks)."""
    import torch
    scene, tris = hall
    rays_np = hall_rays(tris, np.random.default_rng(4))
    w, h, D = 96, 64, 3
    cam = hall_camera(w, h)
    gs = capi.PostSettings()
    dev = torch.device("cuda", 0)
    masks = mesh_bits(12)
    masks[6] = 0  # the largest mesh invisible to queries

    def queries(r, rays, sync):
        return (r.trace_rays(rays, cull="back", mask=0x0F, sync=sync), r.trace_rays(rays, first_hit=True, sync=sync),
                r.trace_occlusion(rays, cull="front", sync=sync), r.trace_rays(rays, sync=sync)) + tuple(
                    r.trace_rays_multi(rays, 16, counts=True, cull="front", mask=0xF0, sync=sync))

    def run(query):
        r = context(scene, bluenoise=bluenoise)
        try:
            r.set_resolution(w, h)
            r.set_camera(cam)
            r.set_prev_camera(cam)
            r.set_batch_paths(w * h)  # one frame per batch: the batches alternate between two lanes
            rays = torch.as_tensor(rays_np, device=dev)
            torch.cuda.synchronize()
            lanes = []
            r.render(0, 4, D, capi.RENDER_AOV)
            lanes.append(r.debug_get(capi.Renderer.DEBUG_LANES_USED))
            q = None
            if query:
                r.set_instance_masks(masks)
                q = queries(r, rays, False)
            r.render(4, 4, D, capi.RENDER_AOV)
            lanes.append(r.debug_get(capi.Renderer.DEBUG_LANES_USED))
            assert lanes == [2, 2]
            r.post_frame(gs, 7, cam)
            r.sync()
            if query:
                q = tuple(bits(x.cpu().numpy()) if x.dtype == torch.float32 else x.cpu().numpy() for x in q)
            s = r.stats()
            out = {"accum": bits(r.readback(capi.BUF_ACCUM_SUM)), "post": bits(r.post_readback()),
                   "stats": tuple(getattr(s, n) for n in STAT_COUNTERS)}
            for kind in (capi.BUF_GBUFFER_GEO, capi.BUF_DIRECT, capi.BUF_ALBEDO, capi.BUF_NORMAL_DEPTH, capi.BUF_INDIRECT):
                out[kind] = bits(r.readback(kind))
            return out, q
        finally:
            r.close()

    a, q = run(True)
    b, _ = run(False)
    for k in b:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "differs after the filtered queries: %s" % (k,)
    assert dict(zip(STAT_COUNTERS, b["stats"]))["rays_primary"] == 8 * w * h
    # and the queries answered as on a context of their own
    r0 = context(scene)
    try:
        r0.set_instance_masks(masks)
        alone = queries(r0, rays_np, True)
        for k, (x, y) in enumerate(zip(q, alone)):
            assert np.array_equal(x, bits(y) if y.dtype == np.float32 else y), "query %d" % k
        hidden = np.isin(q[3][:, 3], np.nonzero(mesh_of_triangles(scene.meshes) == 6)[0])
        assert not hidden.any() and (q[3][:, 3] != MISS).sum() > 0  # the plain call, too, does not see a mesh whose mask is 0
    finally:
        r0.close()
