"""Instanced ray queries on the GPU (cap_instances_set, cap_trace_instances, cap_trace_instances_occlusion): every record, instance
index and occlusion word raw-compared with the box-free brute force of tests/instance_support.py, which runs the oracle's triangle
test on the object-space ray formed from the W the library read back -- no tolerance enters a hit comparison."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from filter_support import mesh_of_triangles, stacked_quads_meshes
from instance_support import (MISS, aimed_rays, bits, candidates, degenerate_rays, expected, extreme_transforms, f32, flatten, grid_rays, grid_scene,
                              instanced_hits, random_rays, regular_transforms, rotation, translations, unit_cube)
from refit_support import Scene, context, cornell_scene

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_STATE = 1, 3
AUTO, LBVH = 0, 1


def live_of(W):
    return ~np.all(W.reshape(len(W), -1) == 0, axis=1)


def check(r, rays, exp, what, **kw):
    """closest records, instance indices and occlusion words of `rays` against the brute force's, raw uint32 compares, every ray"""
    rec, inst, occ, _ = exp
    hits, gi = r.trace_instances(rays, **kw)
    bad = np.flatnonzero(np.any(bits(hits) != rec, axis=1) | (gi.view(np.uint32) != inst))
    assert len(bad) == 0, "%s: %d of %d closest records differ, first ray %d: got %s inst %d, expected %s inst %d" % (
        what, len(bad), len(rays), bad[0], hits[bad[0]], gi[bad[0]], rec[bad[0]].view(f32), np.int32(inst[bad[0]]))
    kw.pop("first_hit", None)
    got = r.trace_instances_occlusion(rays, **kw)
    bad = np.flatnonzero(got != occ)
    assert len(bad) == 0, "%s: %d of %d occlusion words differ, first ray %d" % (what, len(bad), len(rays), bad[0])


# ---- 1. bit-exact against the brute force: regular and extreme transforms, every ray set, two objects, builders, both tree views ----
def object_box(tris):
    return tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)


def make_table():
    M = np.concatenate([regular_transforms(72), extreme_transforms()[0]])
    masks = np.full(len(M), 0xFF, np.uint32)
    masks[5::11] = 0x0F
    masks[7] = 0
    return M, masks


def make_rays(M, tris):
    lo, hi = object_box(tris)
    return np.concatenate([aimed_rays(M, lo, hi, 9), aimed_rays(M[:72], lo, hi, 6, seed=19, distances=(1.0,)), random_rays(900), degenerate_rays()])


@pytest.fixture(scope="module", params=["cube", "quads"])
def instanced(request):
    arrays, tris = unit_cube() if request.param == "cube" else stacked_quads_meshes(12, 0.25, flip_every=3)
    M, masks = make_table()
    rays = make_rays(M, tris)
    assert len(M) >= 64 and len(rays) >= 2000
    return dict(name=request.param, scene=Scene(*arrays), tris=tris, mot=mesh_of_triangles(arrays[4]), M=M, masks=masks, rays=rays, exp=None, W=None)


@pytest.mark.parametrize("no_wide", (0, 1))
@pytest.mark.parametrize("build", (AUTO, LBVH))
def test_bit_exact_against_brute_force(native_lib, instanced, build, no_wide):
    s = instanced
    r = context(s["scene"], build)
    try:
        r.debug_switch("CAP_NO_WIDE8", no_wide)
        info = r.set_instances(s["M"], s["masks"])
        W, boxes = r.instances_readback()
        live = live_of(W)
        must_be_inert = np.r_[np.zeros(72, bool), extreme_transforms()[1]]
        assert info.count == len(s["M"]) and info.inert == int((~live).sum()) and info.tlas_depth >= 7
        assert np.all(live[:72]), "every regular transform must be live"
        assert not np.any(live[must_be_inert]), "singular and non-finite transforms are inert"
        if s["exp"] is None:  # the brute force depends on W alone: once per object
            s["W"], s["exp"] = W, expected(s["rays"], W, live, s["masks"], s["tris"], s["mot"])
            rec, inst, occ, lists = s["exp"]
            n_hit = int((inst != MISS).sum())
            print("%s: %d rays, %d hit, %d occluded, %d with >= 2 instances hit, %d equal-t pairs" % (
                s["name"], len(rec), n_hit, int(occ.sum()), sum(1 for h in lists if len({x[3] for x in h}) >= 2),
                sum(1 for h in lists for a, b in zip(h, h[1:]) if a[0] == b[0])))
            assert n_hit > len(rec) // 4 and sum(1 for h in lists if len({x[3] for x in h}) >= 2) > 100
            assert not np.any(np.isin(inst, np.flatnonzero(~live))), "an inert instance is never hit"
        assert np.array_equal(bits(W), bits(s["W"])), "W does not depend on the builder"
        check(r, s["rays"], s["exp"], "%s builder %d no_wide8 %d" % (s["name"], build, no_wide))
    finally:
        r.close()


def test_many_instances_take_the_sorted_tree(native_lib):
    """3 000 instances (radix-sorted Morton order, a 12-level tree) against the brute force"""
    arrays, tris = unit_cube()
    rng = np.random.default_rng(31)
    n = 3000
    M = np.stack([np.c_[rotation(rng) * rng.uniform(0.5, 2.0), rng.uniform(-60, 60, 3)] for _ in range(n)]).astype(f32)
    rays = np.concatenate([aimed_rays(M[::3], (0, 0, 0), (1, 1, 1), 1, seed=33, distances=(1.0, 100.0)), random_rays(500, 70.0, seed=34)])
    r = context(Scene(*arrays))
    try:
        info = r.set_instances(M)
        assert info.inert == 0 and info.tlas_depth == 13
        W, _ = r.instances_readback()
        check(r, rays, expected(rays, W, live_of(W), None, tris), "3000 instances")
    finally:
        r.close()


# ---- 2. W and the world boxes ----
def test_world_to_object_and_boxes(native_lib, instanced):
    s = instanced
    r = context(s["scene"])
    try:
        r.set_instances(s["M"], s["masks"])
        W, boxes = r.instances_readback()
        live = live_of(W)
        P = s["scene"].positions.astype(np.float64)
        for i in range(72):
            A = np.vstack([s["M"][i].astype(np.float64), [0, 0, 0, 1]])
            inv = np.linalg.inv(A)[:3]
            err = np.abs(W[i].astype(np.float64) - inv)
            bound = 2.0 ** -24 * np.abs(inv) + 1e-12 * np.abs(inv).max()
            assert np.all(err <= bound), (i, err.max(), (err / bound).max())
            img = P @ A[:3, :3].T + A[:3, 3]
            assert np.all(img >= boxes[i, 0]) and np.all(img <= boxes[i, 1]), "world box %d does not contain the image of a vertex" % i
        assert np.all(np.isinf(boxes[~live])), "an inert instance has an empty box"
    finally:
        r.close()


# ---- 3. the exact flattening identity ----
def test_exact_flattening_identity(native_lib):
    arrays, tris = grid_scene(30)
    T = len(tris)
    tr = np.array([[0, 0, 0], [16, 0, 0], [0, 0, 0], [-32, 16, 48], [64, -64, 16], [16, 0, 0], [-64, 64, -64]], f32)  # coinciding copies
    rays = np.concatenate([grid_rays(4000, tr), degenerate_rays()])
    a = context(Scene(*arrays))
    b = context(Scene(*flatten(arrays, tr)))
    try:
        info = a.set_instances(translations(tr))
        assert info.inert == 0
        W, _ = a.instances_readback()
        assert np.array_equal(W, translations(-tr))
        hits, inst = a.trace_instances(rays)
        flat = b.trace_rays(rays)
        hb, fb = bits(hits), bits(flat)
        assert np.array_equal(hb[:, :3], fb[:, :3]), "t, u, v differ from the flattened scene's"
        miss = fb[:, 3] == MISS
        assert np.array_equal(hb[:, 3] == MISS, miss) and np.all(inst[miss] == -1)
        assert np.array_equal(inst[~miss].astype(np.int64) * T + hb[~miss, 3], fb[~miss, 3].astype(np.int64))
        assert (~miss).sum() > 1500 and np.isin(fb[~miss, 3] // T, (0, 1)).sum() > 500  # ties between coinciding copies go to the lower
        assert np.array_equal(a.trace_instances_occlusion(rays), b.trace_occlusion(rays))
    finally:
        a.close()
        b.close()


# ---- 4. filters ----
@pytest.fixture(scope="module")
def small():
    arrays, tris = unit_cube()
    M = regular_transforms(24, seed=41, spread=4.0)
    M[5] = np.c_[np.diag([-1.0, 1, 1]), [1, 0, 0]]  # mirrors, one on top of an unmirrored copy
    M[11] = np.c_[np.eye(3), [0, 0, 0]]
    rays = np.concatenate([aimed_rays(M, (0, 0, 0), (1, 1, 1), 8, seed=42, distances=(1.0, 100.0)), random_rays(200, 6.0, seed=43)])
    return Scene(*arrays), tris, mesh_of_triangles(arrays[4]), M.astype(f32), rays


def test_filters(native_lib, small):
    scene, tris, mot, M, rays = small
    r = context(scene)
    try:
        r.set_instances(M)
        W, _ = r.instances_readback()
        live = live_of(W)
        assert live.all()
        cands = candidates(rays, W, live, tris)
        mesh_bits = (1 << np.arange(6)).astype(np.uint8)
        eight = (1 << (np.arange(len(M)) % 8)).astype(np.uint32)  # eight objects packed as meshes: an instance shows its bit's mesh
        zero = np.full(len(M), 0xFF, np.uint32)
        zero[::2] = 0
        cases = [(None, None, None, None), (None, None, "back", None), (None, None, "front", None), (eight, None, None, 0x15),
                 (eight, mesh_bits, None, None), (eight, mesh_bits, "back", 0x33), (zero, None, None, None), (zero, mesh_bits, "front", 0x0F)]
        for im, mm, cull, mask in cases:
            r.set_instances(M, im)
            r.set_instance_masks(mm)
            what = "instance masks %s mesh masks %s cull %s mask %s" % (im is not None, mm is not None, cull, mask)
            exp = expected(rays, W, live, im, tris, mot, mm, cull, mask, cands)
            check(r, rays, exp, what, cull=cull, mask=mask)
            # ACCEPT_FIRST_HIT: some member of the set, a miss exactly when it is empty
            hits, gi = r.trace_instances(rays, cull=cull, mask=mask, first_hit=True)
            for k, h in enumerate(exp[3]):
                got = (bits(hits[k])[0], bits(hits[k])[1], bits(hits[k])[2], int(np.uint32(gi[k])), int(bits(hits[k])[3]))
                if not h:
                    assert got[3] == MISS and got[4] == MISS and hits[k, 0] == rays[k, 7], (what, k)
                else:
                    assert got in {(bits(t)[0], bits(u)[0], bits(v)[0], i, g) for t, u, v, i, g in h}, (what, k)
        if True:
            # mirrored instance 5 on top of instance 11: cull back keeps the outward faces in both (facing is the object-space one)
            exp = expected(rays, W, live, None, tris, mot, None, "back", None, cands)
            assert sum(1 for h in exp[3] if any(x[3] == 5 for x in h)) > 5
        import torch
        rt = torch.as_tensor(rays, device="cuda:0")
        out = torch.full((len(rays), 4), 7.0, device="cuda:0")
        o = capi.TraceOptions(0x30, 0)
        torch.cuda.synchronize()
        assert capi.lib().cap_trace_instances(r.ctx, rt.data_ptr(), len(rays), out.data_ptr(), None, ctypes.byref(o)) == ERR_INVALID_ARG
        assert capi.lib().cap_trace_instances_occlusion(r.ctx, rt.data_ptr(), len(rays), out.data_ptr(), ctypes.byref(o)) == ERR_INVALID_ARG
        r.sync()
        assert torch.all(out == 7.0), "nothing is written on an error"
    finally:
        r.close()


# ---- 5. life cycle ----
def test_life_cycle(native_lib, small):
    import torch
    scene, tris, mot, M, rays = small
    rays = rays[:300]
    dev = torch.device("cuda", 0)
    r = context(scene)
    try:
        rt = torch.as_tensor(rays, device=dev)
        out = torch.empty((len(rays), 4), device=dev)
        torch.cuda.synchronize()
        L = capi.lib()
        assert L.cap_trace_instances(r.ctx, rt.data_ptr(), len(rays), out.data_ptr(), None, None) == ERR_STATE
        assert L.cap_trace_instances_occlusion(r.ctx, rt.data_ptr(), len(rays), out.data_ptr(), None) == ERR_STATE
        assert L.cap_instances_readback(r.ctx, None, None) == ERR_STATE
        d = np.zeros(2, capi.INSTANCE_DESC_DTYPE)
        d["transform"][:] = np.c_[np.eye(3), np.zeros(3)].ravel()
        d["reserved"][1, 2] = 1
        assert L.cap_instances_set(r.ctx, d.ctypes.data, 2, 0, None) == ERR_INVALID_ARG and b"reserved" in L.cap_last_error()
        assert L.cap_instances_set(r.ctx, d.ctypes.data, 2, 2, None) == ERR_INVALID_ARG
        assert L.cap_instances_set(r.ctx, d.ctypes.data, (1 << 24) + 1, 0, None) == ERR_INVALID_ARG
        assert L.cap_instances_set(r.ctx, d.ctypes.data, 2, capi.INSTANCES_DEVICE, None) == ERR_INVALID_ARG  # a host pointer
        # rigid motion: ten frames, every one replaces the table and is bit-exact
        rng = np.random.default_rng(51)
        for frame in range(10):
            Mf = M.copy()
            Mf[:, :, 3] += rng.uniform(-0.5, 0.5, (len(M), 3)).astype(f32) * frame
            info = r.set_instances(Mf)
            assert info.inert == 0
            W, _ = r.instances_readback()
            check(r, rays, expected(rays, W, live_of(W), None, tris), "frame %d" % frame)
        # device descriptors: the same W, boxes and records as host ones
        r.set_instances(M)
        # misaligned or overlapping arrays: refused before anything is launched (csrc/query_ranges.h, tests/test_query_ranges.py)
        n, R, O = len(rays), rt.data_ptr(), out.data_ptr()
        I = torch.empty(n, dtype=torch.int32, device=dev).data_ptr()
        last_ray, last_hit = R + 32 * (n - 1), O + 16 * (n - 1)
        last_flag = O + 16 * ((n - 1) // 4)  # the 16 bytes that hold the last occlusion flag
        closest = lambda rays_p, out_p, inst_p: L.cap_trace_instances(r.ctx, rays_p, n, out_p, inst_p, None)
        occlusion = lambda rays_p, out_p: L.cap_trace_instances_occlusion(r.ctx, rays_p, n, out_p, None)
        for call, args, words in ((closest, (R + 4, O, I), (b"rays", b"aligned")), (closest, (R, O + 4, I), (b"output", b"aligned")),
                                  (closest, (R, O, I + 2), (b"instances", b"aligned")), (closest, (R, last_ray, I), (b"rays", b"output", b"overlap")),
                                  (closest, (last_hit, O, I), (b"rays", b"output", b"overlap")),
                                  (closest, (R, O, last_hit), (b"output", b"instances", b"overlap")),
                                  (occlusion, (R + 4, O), (b"rays", b"aligned")), (occlusion, (R, O + 4), (b"output", b"aligned")),
                                  (occlusion, (R, last_ray), (b"rays", b"output", b"overlap")),
                                  (occlusion, (last_flag, O), (b"rays", b"output", b"overlap"))):
            assert call(*args) == ERR_INVALID_ARG and all(w in L.cap_last_error() for w in words), (args, L.cap_last_error())
        Wh, Bh = r.instances_readback()
        hh, ih = r.trace_instances(rays)
        info = r.set_instances(torch.as_tensor(M, device=dev))
        Wd, Bd = r.instances_readback()
        hd, idd = r.trace_instances(rays)
        assert info.count == len(M) and np.array_equal(bits(Wh), bits(Wd)) and np.array_equal(bits(Bh), bits(Bd))
        assert np.array_equal(bits(hh), bits(hd)) and np.array_equal(ih, idd)
        # a vertex moved outside the old root box: stale until the refit, then hit where only the new bounds reach
        P = scene.positions.copy()
        P[P[:, 0] == 1.0, 0] = 3.0  # the face x = 1 moves to x = 3
        r.update_vertices(P)
        assert L.cap_trace_instances(r.ctx, rt.data_ptr(), len(rays), out.data_ptr(), None, None) == ERR_STATE
        assert L.cap_instances_set(r.ctx, d.ctypes.data, 1, 0, None) == ERR_STATE
        r.refit_bvh()
        W2, B2 = r.instances_readback()
        assert np.array_equal(bits(W2), bits(Wh)) and not np.array_equal(B2, Bh)
        moved = scene.moved(P).triangles()
        A = M[11].astype(np.float64)  # the identity instance: aim at its stretched part from far outside the old boxes
        extra = np.array([[*(A[:, :3] @ [2.5, 0.4, 0.6] + A[:, 3] + [0, 5, 0]), 0, 0, -1, 0, np.inf]], f32)
        rays2 = np.concatenate([rays, extra])
        exp = expected(rays2, W2, live_of(W2), None, moved)
        assert exp[1][-1] != MISS
        check(r, rays2, exp, "after the refit")
        r.build_bvh()  # a rebuild keeps the table too
        check(r, rays2, exp, "after a rebuild")
        # a new scene drops the table
        r.upload_scene(scene.positions, scene.normals, scene.texcoords, scene.indices, scene.meshes)
        r.build_bvh()
        assert L.cap_trace_instances(r.ctx, rt.data_ptr(), len(rays), out.data_ptr(), None, None) == ERR_STATE
        r.set_instances(M)
        r.set_instances(None)
        assert L.cap_trace_instances(r.ctx, rt.data_ptr(), len(rays), out.data_ptr(), None, None) == ERR_STATE
    finally:
        r.close()


def cornell_frame(r, bluenoise, with_queries=None):
    w = h = 64
    r.set_resolution(w, h)
    r.set_camera(capi.cornell_camera(w, h))
    r.render(0, 2, 2, capi.RENDER_AOV)
    q = with_queries() if with_queries else None
    r.render(2, 2, 2, capi.RENDER_AOV)
    r.sync()
    return bits(r.readback(capi.BUF_ACCUM_SUM)), bits(r.readback(capi.BUF_GBUFFER_GEO)), q


# ---- 5b / 6. a render is untouched by the table and by instanced queries enqueued between its calls; so are the plain queries ----
def test_nothing_else_moved(native_lib, bluenoise, cornell_path):
    import torch
    scene, materials = cornell_scene(cornell_path)
    tris = scene.triangles()
    rng = np.random.default_rng(61)
    o = rng.uniform(0.1, 0.9, (500, 3)) * (tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)) + tris.reshape(-1, 3).min(0)
    rays = np.c_[o, np.zeros(500), rng.normal(size=(500, 3)), np.full(500, np.inf)].astype(f32)
    M = regular_transforms(40, seed=62, spread=2.0)
    dev = torch.device("cuda", 0)

    def run(table):
        r = context(scene, bluenoise=bluenoise)
        try:
            rt = torch.as_tensor(rays, device=dev)
            torch.cuda.synchronize()
            if table:
                r.set_instances(M)
            frame = cornell_frame(r, bluenoise, (lambda: (r.trace_instances(rt, sync=False), r.trace_instances_occlusion(rt, sync=False))) if table else None)
            plain = (bits(r.trace_rays(rays)), r.trace_occlusion(rays), bits(r.trace_rays_multi(rays, 4)), bits(r.trace_rays(rays, cull="back")))
            if table:
                (h, i), occ = frame[2]
                W, _ = r.instances_readback()
                exp = expected(rays, W, live_of(W), None, tris)
                assert np.array_equal(bits(h.cpu().numpy()), exp[0]) and np.array_equal(i.cpu().numpy().view(np.uint32), exp[1])
                assert np.array_equal(occ.cpu().numpy(), exp[2])
            return frame[:2], plain
        finally:
            r.close()

    (fa, pa), (fb, pb) = run(True), run(False)
    for x, y in zip(fa + pa, fb + pb):
        assert np.array_equal(x, y), "a call that does not read the instance table changed with one installed"
