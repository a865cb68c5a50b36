"""Sphere sweep queries on the GPU (cap_sweep_spheres): every record compared bit for bit, all eight words, with the numpy float32
brute force of sweep_support.py over every triangle."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from closest_point_support import arrays, assert_records, bits, context, needles, queries, sphere
from multi_hit_support import stacked_quads
from sweep_support import MISS, RADII, soup_case, soup_sweeps, sweep_queries, sweep_scene
from test_sweep_spheres import TRI, degenerate_sweeps, known_records, known_sweeps

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = 1, 3
CANARY = 0x7FC0BEEF  # a NaN pattern no record holds
B = capi.Renderer  # the CapBvhBuild values
f32 = np.float32


def run(r, q, mask=None):
    return r.sweep_spheres(np.ascontiguousarray(q, f32), mask=mask)


def check(tris, q, what, build=None):
    want, _ = sweep_scene(q, tris)
    r = context([tris], build)
    try:
        assert_records(run(r, q), want, what)
    finally:
        r.close()
    return want


# 1. the soup, near the origin and far from it
@pytest.mark.parametrize("offset", (0.0, 4096.0), ids=("near the origin", "near 4 096"))
def test_soup(native_lib, offset):
    tris, q, want = soup_case(offset)
    hit = bits(want)[:, 6] != MISS
    assert 0.2 * len(q) < hit.sum() < 0.9 * len(q)
    r = context([tris])
    try:
        assert_records(run(r, q), want, "soup at %g" % offset)
    finally:
        r.close()


# 2. scenes built against the prune
def test_sphere_from_its_centre_outward_and_from_outside_inward(native_lib):
    """every subtree is almost equally far from the centre; from outside the sweep grazes many boxes before the first contact"""
    rng = np.random.default_rng(41)
    tris = sphere(20, 20)
    d = rng.normal(size=(256, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = sweep_queries(rng.normal(size=(256, 3)) * 1e-3, 0.05, d)
    out[::4, 3] = 0.0
    start = 3.0 * d + rng.normal(size=(256, 3)) * 0.3
    inward = sweep_queries(start, 0.1, -d * (0.5 + rng.random((256, 1))))
    inward[1::4, 7] = 1.5
    q = np.concatenate([out, inward])
    want = check(tris, q, "sphere")
    hit = bits(want)[:, 6] != MISS
    moving = np.arange(256) % 4 != 0  # (radius 0 touches only where the computed centre lies on the triangle exactly)
    assert hit[:256][moving].all() and 150 < hit[256:].sum() < 256


def test_needles(native_lib):
    rng = np.random.default_rng(42)
    tris = needles(rng, 1000)
    q = np.concatenate([soup_sweeps(rng, tris, 171 if k else 170, radius) for k, radius in enumerate(RADII)])
    want = check(tris, q, "needles")
    assert 50 < (bits(want)[:, 6] != MISS).sum() < len(q)


def test_known_answers(native_lib):
    q = known_sweeps()
    r = context([TRI])
    try:
        assert_records(run(r, q), known_records(), "known answers")
    finally:
        r.close()


# 3. ties
@pytest.mark.parametrize("doubled", (False, True), ids=("quads", "every triangle twice"))
def test_ties_go_to_the_lower_id(native_lib, doubled):
    n = 40
    _, tris = stacked_quads(n, 0.25)
    if doubled:
        tris = np.concatenate([tris, tris])
    xy = [(0.5, 0.5), (0.25, 0.25), (0.75, 0.75), (0.5, 0.25), (0.25, 0.5), (0, 0), (1, 1), (1.125, 0.5), (0.5, -0.125)]
    o = [(x, y, z) for x, y in xy for z in (n * 0.25 + 2.0, -2.0)]
    d = [(0, 0, -1 if z > 0 else 1) for _, _, z in o]
    q = np.concatenate([sweep_queries(o, 0.25, d), sweep_queries(o, 0.0, d), sweep_queries([(0.5, 0.5, 1.125), (0.25, 0.75, 3.0)], 0.5, [(1, 0, 0), (0, 0, 0)])])
    want, table = sweep_scene(q, tris)
    winners = bits(want)[:, 6].astype(np.int64)
    hit = winners != MISS
    tied = (table[hit] == table[hit, winners[hit]][:, None]).sum(1)
    assert hit.sum() > 0.8 * len(q) and (tied >= 2).sum() > 0.6 * hit.sum() and (tied >= 4).sum() >= 2
    if doubled:
        assert (winners[hit] < 2 * n).all() and (tied >= 2).all()
    r = context([tris])
    try:
        assert_records(run(r, q), want, "ties")
    finally:
        r.close()


# 4. tmax
def test_tmax_at_the_answer_and_one_ulp_below(native_lib):
    tris, q, want = soup_case(0.0)
    moving = (bits(want)[:, 6] != MISS) & (want[:, 3] > 0)
    q = q[moving][:256].copy()
    at = want[moving][:256, 3]
    r = context([tris])
    try:
        hits = {}
        for name, tmax in (("at", at), ("below", np.nextafter(at, f32(0)))):
            q[:, 7] = tmax
            w, _ = sweep_scene(q, tris)
            hits[name] = bits(w)[:, 6] != MISS
            assert (w[~hits[name], 3] == q[~hits[name], 7]).all(), "the miss record carries tmax"
            assert_records(run(r, q), w, "tmax " + name)
        assert hits["at"].all() and hits["below"].sum() < 0.5 * len(q), "t <= tmax is inclusive, and the first contact is the first"
    finally:
        r.close()


# 5. degenerate sweeps
def test_degenerate_sweeps_between_good_ones(native_lib):
    import torch
    tris, q, _ = soup_case(0.0)
    bad = degenerate_sweeps()
    q = q[:20 * len(bad)].copy()
    q[3::20] = bad
    want, _ = sweep_scene(q, tris)
    miss = np.zeros(8, np.uint32)
    miss[6] = MISS
    assert (bits(want)[3::20] == miss).all() and (bits(want)[:, 6] != MISS).sum() > 20
    dev = torch.device("cuda", 0)
    out = torch.full((len(q) + 4, 8), CANARY, dtype=torch.int32, device=dev).view(torch.float32)
    r = context([tris])
    try:
        r.sweep_spheres(torch.as_tensor(q, device=dev), out=out[:len(q)])
        got = out.cpu().numpy()
        assert_records(got[:len(q)], want, "degenerate sweeps")
        assert (bits(got[len(q):]) == CANARY).all()
    finally:
        r.close()


# 6. sizes, and the smallest trees
@pytest.fixture(scope="module")
def small_case():
    """64 triangles of the soup and 512 sweeps; the brute force, once"""
    rng = np.random.default_rng(43)
    tris = soup_case(0.0)[0][:64]
    q = np.concatenate([soup_sweeps(rng, tris, 256, radius) for radius in (0.1, 0.3)])
    want, _ = sweep_scene(q, tris)
    assert 100 < (bits(want)[:, 6] != MISS).sum() < 500
    return tris, q, want


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_sizes_with_canaries(native_lib, small_case, n):
    import torch
    tris, q, want = small_case
    reps = -(-n // len(q))
    qn, wn = np.tile(q, (reps, 1))[:n], np.tile(want, (reps, 1))[:n]
    dev = torch.device("cuda", 0)
    out = torch.full((n + 8, 8), CANARY, dtype=torch.int32, device=dev).view(torch.float32)
    r = context([tris])
    try:
        r.sweep_spheres(torch.as_tensor(qn, device=dev), out=out[:n])
        got = out.cpu().numpy()
        assert_records(got[:n], wn, "n = %d" % n)
        assert (bits(got[n:]) == CANARY).all(), "nothing behind the last record"
    finally:
        r.close()


@pytest.mark.parametrize("count", (1, 2, 3))
def test_smallest_scenes(native_lib, small_case, count):
    """one triangle (the root is a leaf), two (one node, one traversal leaf) and three"""
    tris, q, _ = small_case
    few = tris[:count]
    rng = np.random.default_rng(44)
    q = soup_sweeps(rng, few, 256, 0.3)
    want, _ = sweep_scene(q, few)
    hit = bits(want)[:, 6] != MISS
    assert 20 < hit.sum() < 256
    r = context([few])
    try:
        assert r.bvh_info().triangle_count == count
        assert_records(run(r, q), want, "%d triangles" % count)
    finally:
        r.close()


# 7. builders
@pytest.mark.parametrize("build", (B.BVH_BUILD_LBVH, B.BVH_BUILD_SAH, B.BVH_BUILD_PLOC, B.BVH_BUILD_SAH_DEVICE, B.BVH_BUILD_AUTO),
                         ids=("lbvh", "sah", "ploc", "sah_device", "auto"))
def test_every_builder_equals_the_brute_force(native_lib, build):
    tris, q, want = soup_case(0.0)
    r = context([tris], build)
    try:
        assert_records(run(r, q[:1024]), want[:1024], "builder %d" % build)
    finally:
        r.close()


# 8. masks and refused options
def test_masks_and_option_errors(native_lib):
    import torch
    tris, q, want_all = soup_case(0.0)
    q, want_all = q[:512], want_all[:512]
    a, b = tris[:500], tris[500:]
    in_a = np.arange(len(tris)) < 500
    want_a, _ = sweep_scene(q, tris, in_a)
    want_b, _ = sweep_scene(q, tris, ~in_a)
    assert not np.array_equal(bits(want_a), bits(want_b)) and (bits(want_b)[:, 6][bits(want_b)[:, 6] != MISS] >= 500).all()
    dev = torch.device("cuda", 0)
    r = context([a, b])
    try:
        assert_records(run(r, q), want_all, "two meshes, no table")
        r.set_instance_masks([0x01, 0x02])
        assert_records(run(r, q), want_all, "plain call, both masks non-zero")
        assert_records(run(r, q, mask=0x01), want_a, "mask 1")
        assert_records(run(r, q, mask=0x02), want_b, "mask 2")
        assert_records(run(r, q, mask=0x03), want_all, "mask 3")
        assert_records(run(r, q, mask=0xFC), sweep_scene(q, tris, np.zeros(len(tris), bool))[0], "a mask nothing passes")
        r.set_instance_masks([0x00, 0xFF])
        assert_records(run(r, q), want_b, "a mesh with mask 0 is invisible to the plain call")
        r.set_instance_masks(None)
        assert_records(run(r, q, mask=0x01), want_all, "no table: every mesh passes every mask")

        # options the call refuses: nothing is written
        L = capi.lib()
        sw = torch.as_tensor(q, device=dev).contiguous()
        out = torch.full((len(q), 8), CANARY, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        call = lambda *o: L.cap_sweep_spheres(r.ctx, sw.data_ptr(), len(q), out.data_ptr(), ctypes.byref(capi.TraceOptions(o[0], o[1], (ctypes.c_uint32 * 2)(*o[2:]))))
        for flags in (0x04, 0x10, 0x20, 0x01, 0x80000000):
            assert call(flags, 0, 0, 0) == ERR_INVALID_ARG and b"ray_flags" in L.cap_last_error()
        assert call(0, 0, 1, 0) == ERR_INVALID_ARG and call(0, 0, 0, 7) == ERR_INVALID_ARG and b"reserved" in L.cap_last_error()
        assert call(0, 0x100, 0, 0) == ERR_INVALID_ARG and call(0, 0xFFFFFFFF, 0, 0) == ERR_INVALID_ARG
        r.sync()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all())
        assert call(0, 0, 0, 0) == 0  # the all-zero options are the plain call
        r.sync()
        assert_records(out.view(torch.float32).cpu().numpy(), want_all, "all-zero options")
        with pytest.raises(capi.CapError):
            r.sweep_spheres(q, mask=0x100)
    finally:
        r.close()


# 9. refit
def test_stale_until_refit_then_the_moved_vertices(native_lib):
    tris, q, want = soup_case(0.0)
    q, want = q[:512], want[:512]
    rng = np.random.default_rng(3)
    P = arrays(tris)[0]
    moved = (P + f32([0.05, -0.02, 0.03]) + (rng.random(P.shape) - 0.5).astype(f32) * f32(0.02)).astype(f32)
    want_moved, _ = sweep_scene(q, moved.reshape(-1, 3, 3))
    assert not np.array_equal(bits(want_moved), bits(want))
    r = context([tris])
    try:
        assert_records(run(r, q), want, "before the update")
        r.update_vertices(positions=moved)
        with pytest.raises(capi.CapError, match="status 3.*cap_bvh_refit"):
            run(r, q)
        r.refit_bvh()
        assert_records(run(r, q), want_moved, "after the refit")
        r.build_bvh()
        assert_records(run(r, q), want_moved, "after a rebuild")
    finally:
        r.close()


# 10. errors and state, in cap_closest_points' order
def test_argument_and_state_contract(native_lib, small_case):
    import torch
    tris, q, want = small_case
    dev = torch.device("cuda", 0)
    L = capi.lib()
    n = 128
    sw = torch.as_tensor(q[:n], device=dev).contiguous()
    out = torch.full((n + 8, 8), CANARY, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    P, O = sw.data_ptr(), out.data_ptr()
    r = capi.Renderer(0)
    try:
        call = lambda p=P, m=n, o=O: L.cap_sweep_spheres(r.ctx, p, m, o, None)
        assert call() == ERR_STATE and b"cap_bvh_build" in L.cap_last_error()  # nothing uploaded
        r.upload_scene(*arrays(tris))
        assert call() == ERR_STATE and call(P, 0) == ERR_STATE  # uploaded, not built: the state comes before n == 0
        r.build_bvh()
        assert L.cap_sweep_spheres(None, P, n, O, None) == ERR_INVALID_ARG
        assert call(None) == ERR_INVALID_ARG and call(P, n, None) == ERR_INVALID_ARG and b"NULL" in L.cap_last_error()
        assert call(P + 4) == ERR_INVALID_ARG and b"sweeps is not 16-byte aligned" in L.cap_last_error()
        assert call(P, n, O + 8) == ERR_INVALID_ARG and b"hits is not 16-byte aligned" in L.cap_last_error()
        assert call(P, n, P) == ERR_INVALID_ARG and call(P, n, P + 32 * (n - 1) + 16) == ERR_INVALID_ARG and b"overlap" in L.cap_last_error()
        assert call(O + 32 * (n - 1) + 16, n, O) == ERR_INVALID_ARG
        assert call(P, 1 << 60) == ERR_INVALID_ARG and b"address space" in L.cap_last_error()
        assert call(None, 0, None) == 0  # nothing to do
        r.sync()
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()), "nothing is written on an error"
        assert call() == 0
        r.sync()
        got = out.view(torch.float32).cpu().numpy()
        assert_records(got[:n], want[:n], "the call itself")
        assert (bits(got[n:]) == CANARY).all()
        with pytest.raises(capi.CapError):
            r.sweep_spheres(torch.zeros((4, 4), device=dev))
        with pytest.raises(capi.CapError):
            r.sweep_spheres(sw, out=torch.zeros((n, 4), device=dev))
    finally:
        r.close()


# 11. the contact is the closest-point function's
def test_each_hit_is_what_closest_points_says_at_the_contact_centre(native_lib, small_case):
    """closest_points at c = o + t d (at o itself for t = 0), with the winning triangle alone unmasked, returns the hit's point, u, v and
    feature; its dist2 is within the acceptance bound"""
    tris, q, want = small_case
    r = context([t[None] for t in tris])  # one mesh per triangle
    try:
        rec = run(r, q)
        assert_records(rec, want, "one mesh per triangle")
        ids = bits(rec)[:, 6]
        t = rec[:, 3:4]
        c = np.where(t == 0, q[:, 0:3], q[:, 0:3] + t * q[:, 4:7]).astype(f32)
        seen = 0
        for g in np.unique(ids[ids != MISS]):
            rows = np.nonzero(ids == g)[0]
            masks = np.zeros(len(tris), np.uint8)
            masks[g] = 0xFF
            r.set_instance_masks(masks)
            near = r.closest_points(queries(c[rows]))
            assert np.array_equal(bits(near)[:, [0, 1, 2, 4, 5, 6, 7]], bits(rec)[rows][:, [0, 1, 2, 4, 5, 6, 7]]), g
            r2 = q[rows, 3] * q[rows, 3]
            assert (near[:, 3] <= r2 * (f32(1) + f32(8) * f32(2.0 ** -24))).all()
            seen += len(rows)
        assert seen > 100
    finally:
        r.close()


def test_a_render_is_unchanged_by_a_sweep_between_its_batches(native_lib, bluenoise, cornell_path):
    geo = capi.Geometry(cornell_path)
    cam = capi.cornell_camera(64, 64)
    rng = np.random.default_rng(5)
    d = rng.normal(size=(1000, 3))
    q = sweep_queries(rng.random((1000, 3)) * 600.0 - 20.0, 5.0 + 20.0 * rng.random(1000), d / np.linalg.norm(d, axis=1, keepdims=True))
    result = []
    for interleave in (False, True):
        r = capi.Renderer(0)
        try:
            r.upload_geometry(geo)
            r.upload_bluenoise(bluenoise)
            r.build_bvh()
            r.set_resolution(64, 64)
            r.set_camera(cam)
            r.render(0, 2, 2, capi.RENDER_AOV)
            if interleave:
                before = (bits(r.readback(capi.BUF_ACCUM_SUM)).copy(), r.stats().as_dict())
                rec = r.sweep_spheres(q)
                after = (bits(r.readback(capi.BUF_ACCUM_SUM)), r.stats().as_dict())
                assert np.array_equal(before[0], after[0])
                assert {k: v for k, v in before[1].items() if not k.startswith("ms_")} == {k: v for k, v in after[1].items() if not k.startswith("ms_")}
                P = geo.positions.reshape(-1, 3)
                tris = np.concatenate([P[geo.indices[int(m[3]):int(m[3]) + int(m[2])].astype(np.int64) + int(m[1])].reshape(-1, 3, 3) for m in geo.meshes])
                assert_records(rec, sweep_scene(q, tris)[0], "the Cornell box")
            r.render(2, 2, 2, capi.RENDER_AOV)
            s = r.stats()
            result.append((bits(r.readback(capi.BUF_ACCUM_SUM)), (s.rays_primary, s.rays_extension, s.rays_shadow, s.shaded_vertices, s.frames)))
        finally:
            r.close()
    assert np.array_equal(result[0][0], result[1][0]) and result[0][1] == result[1][1]
