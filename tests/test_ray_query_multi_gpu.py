"""Multi-hit ray queries (cap_trace_rays_multi) on the MI355X.  Every page and count is compared on raw uint32 bits, miss padding
included: against every hit by the oracle's triangle test (stacked quads, Cornell box), against the oracle on float64 candidate
supersets (262 k hall), across the wide and binary kernels and every builder; plus paging to exhaustion, degenerate rays, sizes and
the launch split, the argument contract, vertex updates, and that queries leave a render untouched."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from multi_hit_support import (MISS, all_hits, bits, candidate_superset, expected_pages, hit_list_array, page_to_exhaustion,
                               stacked_quads)
from refit_support import assert_same_render, context, hall_camera, hall_scene, render_result, Scene

pytestmark = pytest.mark.gpu
BUILDERS = (0, 1, 2, 3, 4)
ERR_INVALID_ARG, ERR_STATE = 1, 3
SENTINEL = 0x7FBADBAD


def ray_array(o, tmin, d, tmax):
    r = np.zeros((len(o), 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


def degenerate_rays():
    nan, inf = np.float32("nan"), np.float32("inf")
    base = np.array([0.3, 0.6, -1.0, 0.0, 0.0, 0.0, 1.0, 100.0], np.float32)
    out = []
    for k in range(8):
        r = base.copy()
        r[k] = nan
        out.append(r)
    for k in (0, 1, 2, 4, 5, 6):
        r = base.copy()
        r[k] = inf
        out.append(r)
    r = base.copy()
    r[4:7] = 0.0
    out.append(r)
    for tmin, tmax in ((1.0, 1.0), (2.0, 1.0), (inf, inf)):
        r = base.copy()
        r[3], r[7] = tmin, tmax
        out.append(r)
    return np.array(out, np.float32)


def check_pages(r, rays, lists, ks=(1, 2, 5, 16), what=""):
    for k in ks:
        want, cnt = expected_pages(rays, lists, k)
        got = r.trace_rays_multi(rays, k)
        assert got.shape == (len(rays), k, 4)
        bad = np.nonzero((bits(got) != bits(want)).any((1, 2)))[0]
        assert len(bad) == 0, "%s k=%d: %d rays differ, first %d: got %s want %s" % (what, k, len(bad), bad[0], bits(got[bad[0]]), bits(want[bad[0]]))
        got, c = r.trace_rays_multi(rays, k, counts=True)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(c, cnt), "%s k=%d with counts" % (what, k)
    _, c = r.trace_rays_multi(rays, 0, counts=True)
    assert np.array_equal(c, expected_pages(rays, lists, 0)[1]), what


def check_paging(r, rays, lists, ks=(1, 3, 4), what=""):
    crossed = 0
    for k in ks:
        walked, pages = page_to_exhaustion(r, rays, k)
        for i in range(len(rays)):
            assert np.array_equal(bits(walked[i]), bits(hit_list_array(lists[i]))), "%s k=%d ray %d" % (what, k, i)
            h = lists[i]
            crossed += sum(1 for j in range(k, len(h), k) if h[j - 1][0] == h[j][0])  # an equal-t pair split by a page boundary
    return crossed


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. stacked quads
@pytest.fixture(scope="module")
def quads():
    arrays, tris = stacked_quads(40, 0.25)
    rng = np.random.default_rng(11)
    sets = []
    n = 48
    xy = rng.uniform(0.02, 0.98, (n, 2))
    sets.append(ray_array(np.c_[xy, np.full(n, -0.5)], 0.0, np.tile([0, 0, 1.0], (n, 1)), np.inf))  # through every quad: 40 hits
    s = rng.uniform(0.05, 0.95, n).astype(np.float32)  # on the shared diagonal: equal-t pairs
    sets.append(ray_array(np.c_[s, s, np.full(n, 10.5)], 0.0, np.tile([0, 0, -1.0], (n, 1)), np.inf))
    zs = (rng.integers(0, 39, n) * 0.25 + 0.125).astype(np.float32)  # between quads, both directions, cut intervals
    sgn = rng.choice([-1.0, 1.0], n)
    sets.append(ray_array(np.c_[rng.uniform(0.02, 0.98, (n, 2)), zs], rng.uniform(0, 0.5, n), np.c_[np.zeros((n, 2)), sgn],
                          rng.uniform(0.5, 4.0, n)))
    o = np.c_[rng.uniform(-0.5, 1.5, (n, 2)), rng.uniform(-1, 11, n)]  # slanted, from anywhere
    sets.append(ray_array(o, 0.0, np.c_[rng.normal(size=(n, 2)) * 0.1, rng.choice([-1.0, 1.0], n)], np.inf))
    rays = np.concatenate(sets).astype(np.float32)
    lists = [all_hits(x, tris) for x in rays]
    assert max(len(h) for h in lists) > 16
    ties = sum(1 for h in lists for a, b in zip(h, h[1:]) if a[0] == b[0])
    assert ties > 100
    return Scene(*arrays), tris, rays, lists


@pytest.mark.parametrize("build", BUILDERS)
def test_stacked_quads_brute_force_and_paging(native_lib, quads, build):
    scene, tris, rays, lists = quads
    r = context(scene, build)
    try:
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            assert r.debug_get(capi.Renderer.DEBUG_WIDE_IN_USE) == 1 - no_wide
            what = "builder %d no_wide8 %d" % (build, no_wide)
            check_pages(r, rays, lists, what=what)
            assert check_paging(r, rays, lists, what=what) > 0  # equal-t pairs on both sides of a page boundary
    finally:
        r.close()


# 2. Cornell box
@pytest.fixture(scope="module")
def cornell(cornell_path):
    from refit_support import cornell_scene
    scene, _ = cornell_scene(cornell_path)
    tris = scene.triangles()
    rng = np.random.default_rng(5)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    c = (lo + hi) / 2

    def dirs(n):
        v = rng.normal(size=(n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    sets = [ray_array(rng.uniform(lo + 0.02, hi - 0.02, (3500, 3)), 0.0, dirs(3500), np.where(rng.random(3500) < 0.5, np.inf, 100.0))]
    for radius, n in ((4.0, 1000), (60.0, 300)):  # outside; 60: beyond the wide view's budget, handed to the binary kernel
        o = c + dirs(n) * radius
        sets.append(ray_array(o, 0.0, rng.uniform(lo, hi, (n, 3)) - o, np.inf))
    pts = np.concatenate([tris.reshape(-1, 3), (tris[:, 0] + tris[:, 1]) / 2, (tris[:, 1] + tris[:, 2]) / 2, (tris[:, 0] + tris[:, 2]) / 2])
    for _ in range(6):  # at shared edges and vertices
        o = rng.uniform(lo + 0.05, hi - 0.05, (len(pts), 3)).astype(np.float32)
        sets.append(ray_array(o, 0.0, pts - o, np.inf))
    k = rng.integers(0, len(tris), 1000)  # from surfaces
    b = rng.dirichlet((1, 1, 1), 1000).astype(np.float32)
    o = (tris[k] * b[:, :, None]).sum(1).astype(np.float32)
    for tmin in (0.0, 1e-4):
        sets.append(ray_array(o, tmin, dirs(1000), np.inf))
    rays = np.concatenate(sets).astype(np.float32)
    assert len(rays) >= 7500
    lists = [all_hits(x, tris) for x in rays]
    return scene, tris, rays, lists


def test_cornell_brute_force(native_lib, cornell):
    scene, tris, rays, lists = cornell
    r = context(scene)
    try:
        assert r.debug_get(capi.Renderer.DEBUG_WIDE_IN_USE) == 1
        check_pages(r, rays, lists, ks=(1, 4, 16), what="cornell")
        assert np.array_equal(bits(r.trace_rays_multi(rays, 1)[:, 0]), bits(r.trace_rays(rays)))  # k = 1 is cap_trace_rays
        r.debug_switch("CAP_NO_WIDE8", 1)
        check_pages(r, rays, lists, ks=(4,), what="cornell no_wide8")
    finally:
        r.close()


# 3. the 262 k hall against float64 candidate supersets
@pytest.fixture(scope="module")
def hall():
    s = hall_scene(1.0)
    assert len(s.indices) // 3 > 250000
    return s, s.triangles()


def hall_rays(tris, rng):
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    v = rng.normal(size=(384, 3))
    sets = [ray_array(rng.uniform(lo + 0.01, hi - 0.01, (384, 3)), 0.0, v / np.linalg.norm(v, axis=1, keepdims=True), np.inf)]
    # along the colonnades (columns at z = +-3.4, x in -10.5 .. 10.5): two surfaces per column, then the end wall
    n = 96
    z = rng.choice([-3.4, 3.4], n) + rng.uniform(-0.15, 0.15, n)
    o = np.c_[np.full(n, -11.9), rng.uniform(0.3, 3.8, n), z]
    d = np.c_[np.ones(n), rng.normal(size=(n, 2)) * 0.002]
    sets.append(ray_array(o, 0.0, d / np.linalg.norm(d, axis=1, keepdims=True), np.inf))
    far = (lo + hi) / 2 + rng.normal(size=(32, 3)) * 300.0  # far outside: handed to the binary kernel
    sets.append(ray_array(far, 0.0, rng.uniform(lo, hi, (32, 3)) - far, np.inf))
    return np.concatenate(sets).astype(np.float32)


def test_hall_against_candidates(native_lib, hall):
    scene, tris = hall
    rays = hall_rays(tris, np.random.default_rng(9))
    r = context(scene)
    try:
        assert r.debug_get(capi.Renderer.DEBUG_WIDE_IN_USE) == 1
        page, cnt = r.trace_rays_multi(rays, 16, counts=True)
        cands = candidate_superset(rays, tris)
        lists = []
        for i in range(len(rays)):
            named = [int(g) for g in bits(page[i])[:, 3] if g != MISS]
            lists.append(all_hits(rays[i], tris, cands[i] + named))
        want, wcnt = expected_pages(rays, lists, 16)
        bad = np.nonzero((bits(page) != bits(want)).any((1, 2)))[0]
        assert len(bad) == 0, "%d rays differ, first %d" % (len(bad), bad[0])
        assert np.array_equal(cnt, wcnt)
        # the nearest candidates alone decide the first record (k = 1, i.e. cap_trace_rays)
        near = candidate_superset(rays, tris, nearest=True)
        assert all(set(near[i]) <= set(cands[i]) for i in range(len(rays)))
        first = expected_pages(rays, [all_hits(x, tris, c + [g for g in [int(bits(p)[0, 3])] if g != MISS])
                                      for x, c, p in zip(rays, near, page)], 1)[0]
        assert np.array_equal(bits(first), bits(r.trace_rays_multi(rays, 1))) and np.array_equal(bits(first[:, 0]), bits(r.trace_rays(rays)))
        deep = np.nonzero(wcnt > 16)[0]
        assert len(deep) >= 10 and (wcnt[len(rays) - 128:len(rays) - 32] > 16).sum() > 0  # colonnade rays among them
        walked, _ = page_to_exhaustion(r, rays[deep], 16)
        for j, i in enumerate(deep):
            assert np.array_equal(bits(walked[j]), bits(hit_list_array(lists[i]))), "ray %d" % i
        # the binary kernels and every builder give the same bits
        r.debug_switch("CAP_NO_WIDE8", 1)
        p2, c2 = r.trace_rays_multi(rays, 16, counts=True)
        assert np.array_equal(bits(p2), bits(page)) and np.array_equal(c2, cnt)
        p4 = r.trace_rays_multi(rays, 4)
        assert np.array_equal(bits(p4), bits(page[:, :4]))
    finally:
        r.close()
    for build in (1, 2, 3, 4):
        rb = context(scene, build)
        try:
            p, c = rb.trace_rays_multi(rays, 16, counts=True)
            assert np.array_equal(bits(p), bits(page)) and np.array_equal(c, cnt), "builder %d" % build
        finally:
            rb.close()


# 4. degenerate rays
def test_degenerate_rays(native_lib, quads):
    scene, _, _, _ = quads
    deg = degenerate_rays()
    r = context(scene)
    try:
        for no_wide in (0, 1):
            r.debug_switch("CAP_NO_WIDE8", no_wide)
            for k in (1, 3, 16):
                want = np.zeros((len(deg), k, 4), np.float32)
                want[:, :, 0] = deg[:, 7:8]
                want.view(np.uint32)[:, :, 3] = MISS
                p, c = r.trace_rays_multi(deg, k, counts=True)
                assert np.array_equal(bits(p), bits(want)) and np.all(c == 0)
                garbage = np.ones_like(want)  # a cursor in continue mode is not even read
                p, c = r.trace_rays_multi(deg, k, counts=True, resume=garbage)
                assert np.array_equal(bits(p), bits(want)) and np.all(c == 0)
            _, c = r.trace_rays_multi(deg, 0, counts=True)
            assert np.all(c == 0)
    finally:
        r.close()


# 5. sizes
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sizes_leave_the_rest_untouched(native_lib, quads, n):
    import torch
    scene, tris, rays, lists = quads
    dev = torch.device("cuda", 0)
    sel = np.arange(n) % len(rays)
    r = context(scene)
    try:
        buf = torch.full(((n + 8) * 3, 4), SENTINEL, dtype=torch.int32, device=dev)
        cnt = torch.full((n + 16,), SENTINEL, dtype=torch.int32, device=dev)
        t = torch.as_tensor(rays[sel], device=dev)
        L = capi.lib()
        assert L.cap_trace_rays_multi(r.ctx, t.data_ptr(), n, 3, buf.data_ptr(), cnt.data_ptr(), 0) == 0
        r.sync()
        b, c = buf.cpu().numpy(), cnt.cpu().numpy()
        assert np.all(b[3 * n:] == SENTINEL) and np.all(c[n:] == SENTINEL)
        want, wc = expected_pages(rays[sel], [lists[i] for i in sel], 3)
        assert np.array_equal(b[:3 * n].reshape(n, 3, 4).view(np.uint32), bits(want)) and np.array_equal(c[:n], wc)
    finally:
        r.close()


def test_launch_split(native_lib, quads):
    import torch
    scene, tris, rays, lists = quads
    dev = torch.device("cuda", 0)
    n = (1 << 24) + 5
    r = context(scene)
    try:
        t = torch.as_tensor(rays, device=dev).repeat((n + len(rays) - 1) // len(rays), 1)[:n].contiguous()
        buf = torch.full((n + 4, 4), SENTINEL, dtype=torch.int32, device=dev)
        L = capi.lib()
        assert L.cap_trace_rays_multi(r.ctx, t.data_ptr(), n, 1, buf.data_ptr(), None, 0) == 0
        one = r.trace_rays(t)
        r.sync()
        assert torch.equal(buf[:n], one.view(torch.int32)) and bool((buf[n:] == SENTINEL).all())
        del one
        cnt = torch.full((n + 4,), SENTINEL, dtype=torch.int32, device=dev)
        assert L.cap_trace_rays_multi(r.ctx, t.data_ptr(), n, 0, None, cnt.data_ptr(), 0) == 0
        r.sync()
        wc = torch.as_tensor(np.array([len(h) for h in lists], np.int32), device=dev).repeat((n + len(rays) - 1) // len(rays))[:n]
        assert torch.equal(cnt[:n], wc) and bool((cnt[n:] == SENTINEL).all())
    finally:
        r.close()


# 6. the argument contract
def test_argument_contract(native_lib, quads):
    import torch
    scene, _, _, _ = quads
    dev = torch.device("cuda", 0)
    L = capi.lib()
    rays = torch.zeros((128, 8), dtype=torch.float32, device=dev)
    rays[:, 0:2] = 0.3
    rays[:, 2] = -1.0
    rays[:, 6] = 1.0
    rays[:, 7] = 100.0
    hits = torch.full((128 * 16 + 8, 4), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((136,), SENTINEL, dtype=torch.int32, device=dev)
    R, H, C = rays.data_ptr(), hits.data_ptr(), cnt.data_ptr()
    r = capi.Renderer(0)
    try:
        r.upload_scene(scene.positions, scene.normals, scene.texcoords, scene.indices, scene.meshes)
        f = lambda *a: L.cap_trace_rays_multi(r.ctx, *a)
        assert f(R, 128, 4, H, C, 0) == ERR_STATE  # before cap_bvh_build
        r.build_bvh()
        assert f(R, 128, 17, H, C, 0) == ERR_INVALID_ARG  # k > CAP_MULTI_MAX_K
        assert f(R, 128, 0, H, C, 0) == ERR_INVALID_ARG and f(R, 128, 0, None, None, 0) == ERR_INVALID_ARG  # k = 0
        assert f(R, 128, 0, None, C, 1) == ERR_INVALID_ARG  # CONTINUE with k = 0
        assert f(R, 128, 4, H, C, 2) == ERR_INVALID_ARG and f(R, 128, 4, H, C, 0x80000000) == ERR_INVALID_ARG  # unknown flags
        assert f(None, 128, 4, H, C, 0) == ERR_INVALID_ARG and f(R, 128, 4, None, C, 0) == ERR_INVALID_ARG  # NULL
        assert f(R + 4, 64, 4, H, C, 0) == ERR_INVALID_ARG and f(R, 64, 4, H + 8, C, 0) == ERR_INVALID_ARG  # misaligned
        assert f(R, 64, 4, H, C + 2, 0) == ERR_INVALID_ARG
        assert f(R, 128, 4, R + 32 * 64, C, 0) == ERR_INVALID_ARG  # hits over rays
        assert f(R, 128, 4, H, R + 32 * 127, 0) == ERR_INVALID_ARG  # counts over rays
        assert f(R, 128, 4, H, H + 16 * 4 * 127 + 12, 0) == ERR_INVALID_ARG  # counts over hits
        assert f(R, 1 << 58, 16, H, None, 0) == ERR_INVALID_ARG  # 2^58 rays fit (2^63 B), their 2^58 x 16 records do not
        assert L.cap_trace_rays_multi(None, R, 1, 1, H, C, 0) == ERR_INVALID_ARG
        assert f(R, 0, 4, H, C, 0) == 0  # nothing to do
        r.sync()
        torch.cuda.synchronize()
        assert bool((hits == SENTINEL).all()) and bool((cnt == SENTINEL).all())  # nothing was written
        # the binding's own checks
        with pytest.raises(capi.CapError):
            r.trace_rays_multi(rays, 17)
        with pytest.raises(capi.CapError):
            r.trace_rays_multi(rays, 0)
        with pytest.raises(capi.CapError):
            r.trace_rays_multi(rays, 4, resume=torch.zeros((128, 3, 4), dtype=torch.float32, device=dev))
        p = r.trace_rays_multi(rays, 4)
        again = r.trace_rays_multi(rays, 4, resume=p)
        assert again.data_ptr() == p.data_ptr()  # continued in place
    finally:
        r.close()


# 7. vertex updates
def test_vertex_updates(native_lib, quads):
    scene, tris, rays, lists = quads
    P = scene.positions.astype(np.float64)
    moved = P.copy()
    moved[:, 0] += 0.1 * np.sin(3 * P[:, 2])  # shear the stack
    moved[:, 2] *= 1.5
    moved = moved.astype(np.float32)
    r = context(scene)
    try:
        r.update_vertices(positions=moved)
        with pytest.raises(capi.CapError, match="vertices changed"):
            r.trace_rays_multi(rays, 4)
        r.refit_bvh()
        fresh = context(scene.moved(positions=moved))
        try:
            for no_wide in (0, 1):
                r.debug_switch("CAP_NO_WIDE8", no_wide)
                fresh.debug_switch("CAP_NO_WIDE8", no_wide)
                for k in (1, 5, 16):
                    a, ca = r.trace_rays_multi(rays, k, counts=True)
                    b, cb = fresh.trace_rays_multi(rays, k, counts=True)
                    assert np.array_equal(bits(a), bits(b)) and np.array_equal(ca, cb)
            mtris = scene.moved(positions=moved).triangles()
            want, wc = expected_pages(rays, [all_hits(x, mtris) for x in rays], 16)
            assert np.array_equal(bits(a), bits(want)) and np.array_equal(ca, wc)
        finally:
            fresh.close()
    finally:
        r.close()


# 8. a render interrupted by multi-hit queries is unchanged
STAT_COUNTERS = [n for n, t in capi.Stats._fields_ if t is ctypes.c_uint64]  # every counter of CapStats (the ms_* fields are timings)


@pytest.mark.parametrize("feedback", [False, True])
def test_queries_do_not_interfere_with_rendering(native_lib, bluenoise, hall, feedback):
    """Frames 0-3 on two batch lanes, multi-hit queries enqueued behind them while they run (device rays, no host sync), frames 4-7
    into the same accumulation: accumulation, post output, AOV planes and every CapStats counter equal a run without the queries."""
    import torch
    scene, tris = hall
    rays_np = hall_rays(tris, np.random.default_rng(4))
    w, h, D = 96, 64, 3
    cam = hall_camera(w, h)
    gs = capi.PostSettings()
    dev = torch.device("cuda", 0)

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

            def frames(f0):
                if feedback:
                    for f in range(f0, f0 + 4):
                        r.render(f, 1, D, capi.RENDER_AOV | capi.RENDER_GBUFFER_FEEDBACK)
                        r.post_frame(gs, f, cam)
                else:
                    r.render(f0, 4, D, capi.RENDER_AOV)
                    lanes.append(r.debug_get(capi.Renderer.DEBUG_LANES_USED))

            frames(0)
            q = None
            if query:  # enqueued on the context stream behind the frames still in flight, no host sync in between
                p16, c16 = r.trace_rays_multi(rays, 16, counts=True, sync=False)
                _, c0 = r.trace_rays_multi(rays, 0, counts=True, sync=False)
                first = r.trace_rays_multi(rays, 4, sync=False)
                second = r.trace_rays_multi(rays, 4, resume=r.trace_rays_multi(rays, 4, sync=False), sync=False)
                q = (p16, c16, c0, first, second)
            frames(4)
            if not feedback:
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
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "differs after the queries: %s" % (k,)
    assert dict(zip(STAT_COUNTERS, b["stats"]))["rays_primary"] == 8 * w * h
    # and the queries answered as on a context of their own
    r0 = context(scene)
    try:
        p16, c16 = r0.trace_rays_multi(rays_np, 16, counts=True)
        _, c0 = r0.trace_rays_multi(rays_np, 0, counts=True)
        p4 = r0.trace_rays_multi(rays_np, 4)
        nxt = r0.trace_rays_multi(rays_np, 4, resume=p4.copy())
        assert np.array_equal(q[0], bits(p16)) and np.array_equal(q[1], c16) and np.array_equal(q[2], c0)
        assert np.array_equal(q[3], bits(p4)) and np.array_equal(q[4], bits(nxt))
    finally:
        r0.close()
