"""Multi-hit instanced ray queries on the GPU (cap_trace_instances_multi): every page, instance page and count raw-compared, as uint32
words and for every ray, with the box-free brute force of tests/instance_support.py (instanced_hits: the oracle's triangle test on the
object-space ray formed from the W the library read back), turned into pages, cursors and counts by tests/instance_multi_support.py.
No tolerance enters a comparison."""
import ctypes

import numpy as np
import pytest

from capsaicin_amd import capi
from filter_support import mesh_of_triangles, stacked_quads_meshes
from instance_multi_support import expected_pages, listed, words
from instance_support import (MISS, aimed_rays, bits, candidates, degenerate_rays, expected, extreme_transforms, f32, flatten, grid_rays, grid_scene,
                              random_rays, regular_transforms, translations, unit_cube)
from object_support import concat, object_candidates, scene_triangles, single_triangle, triangle_ranges
from object_support import expected as object_expected
from refit_support import Scene, context, cornell_scene

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_STATE = 1, 3
AUTO, LBVH = 0, 1
KS = (1, 2, 4, 5, 8, 16)  # every bucket (1, 4, 8, 16) and k strictly inside one (2, 5)


def live_of(W):
    return ~np.all(W.reshape(len(W), -1) == 0, axis=1)


def compare(out, exp, counts, what):
    """hit page, instance page and (counts=True) counts of one call against the expected words, every ray"""
    rec, inst, cnt = exp
    h, gi = np.asarray(out[0].cpu() if hasattr(out[0], "cpu") else out[0]), np.asarray(out[1].cpu() if hasattr(out[1], "cpu") else out[1])
    assert h.shape == rec.shape and gi.shape == inst.shape, (what, h.shape, gi.shape)
    bad = np.flatnonzero(np.any(bits(h).reshape(len(rec), -1) != rec.reshape(len(rec), -1), axis=1) | np.any(gi.view(np.uint32) != inst, axis=1))
    assert len(bad) == 0, "%s: %d of %d pages differ, first ray %d:\ngot %s\ninst %s\nexpected %s\ninst %s" % (
        what, len(bad), len(rec), bad[0], h[bad[0]], gi[bad[0]], rec[bad[0]].view(f32), inst[bad[0]].view(np.int32))
    if counts:
        c = np.asarray(out[2].cpu() if hasattr(out[2], "cpu") else out[2])
        bad = np.flatnonzero(c.view(np.uint32) != cnt)
        assert len(bad) == 0, "%s: %d of %d counts differ, first ray %d: got %d, expected %d" % (what, len(bad), len(cnt), bad[0], c[bad[0]], cnt[bad[0]])


def check_pages(r, rays, lists, what, ks=KS, **kw):
    """first pages for every k with and without counts (the pruned and the counting kernels), and k = 0: counts only"""
    for k in ks:
        exp = expected_pages(lists, rays, k)
        for counts in (False, True):
            compare(r.trace_instances_multi(rays, k, counts=counts, **kw), exp, counts, "%s k %d counts %s" % (what, k, counts))
    compare(r.trace_instances_multi(rays, 0, counts=True, **kw), expected_pages(lists, rays, 0), True, "%s counts only" % what)


def check_paging(r, rays, lists, k, counts, what, **kw):
    """pages with CAP_MULTI_CONTINUE until every page is empty, each compared, then one call more; the concatenation is the list"""
    import torch
    rt = torch.as_tensor(rays, device="cuda:0")
    longest = max(len(h) for h in lists)
    pages = -(-longest // k)  # calls that return something; call `pages` is empty for every ray, call `pages + 1` the one after the end
    got = [[] for _ in lists]
    resume = None
    for step in range(pages + 2):
        out = r.trace_instances_multi(rt, k, counts=counts, resume=resume, **kw)
        resume = (out[0], out[1])
        exp = expected_pages(lists, rays, k, step * k)
        compare(out, exp, counts, "%s k %d page %d" % (what, k, step))
        if step < pages:
            hh, ii = bits(out[0].cpu().numpy()), out[1].cpu().numpy().view(np.uint32)
            for j in np.flatnonzero(ii[:, 0] != MISS):
                got[j] += listed(hh[j], ii[j])
    assert step == pages + 1 and np.all(resume[1].cpu().numpy() == -1), "the call after the end returns miss pages"
    for j, h in enumerate(lists):
        assert got[j] == words(h), "%s k %d: ray %d's pages do not add up to its hit list" % (what, k, j)


# ---- the table and rays of tests 1, 2, 3 ----
# regular_transforms(24, spread=4.0) + extreme_transforms(), and exact copies of four regular instances behind them: coinciding copies
# have the same W, hence the same object-space ray and the same t, so every pair in one of them ties with its twin's.
# Rays from random directions (aimed_rays, random_rays) seldom run along a stack of quads: measured on the CPU brute force, 4 of 859
# had more than 16 pairs and 4 an equal-t pair, whatever the seeds.  axis_rays adds rays along the objects' z axis, most of them
# through the copied instances (12 quads x 2 coinciding instances = 24 pairs, twelve ties).
N_REGULAR = 24
COPIED = (1, 2, 4, 5)  # a rotation, a scaled rotation, a shear, a mirror


def make_table():
    M = np.concatenate([regular_transforms(N_REGULAR, spread=4.0), extreme_transforms()[0]])
    M = np.concatenate([M, M[list(COPIED)]])
    masks = np.full(len(M), 0xFF, np.uint32)
    masks[3::7] = 0x0F
    masks[9] = 0x31
    masks[6] = 0
    return M, masks


def axis_rays(M, lo, hi, per_instance, seed):
    """rays along each instance's object-space z axis, tilted a little, through the middle half of the object's x-y extent"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    rays = []
    for A in np.asarray(M, np.float64):
        for _ in range(per_instance):
            p = lo + (hi - lo) * [rng.uniform(0.25, 0.75), rng.uniform(0.25, 0.75), -0.5]
            d = np.array([rng.normal() * 0.02, rng.normal() * 0.02, 1.0]) * (hi[2] - lo[2]) * rng.uniform(0.5, 2.0)
            rays.append(np.array([*(A[:, :3] @ p + A[:, 3]), 0.0, *(A[:, :3] @ d), np.inf], f32))
    return np.array(rays, f32)


def make_rays(M, tris):
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    rays = np.concatenate([aimed_rays(M, lo, hi, 7), aimed_rays(M[:N_REGULAR], lo, hi, 4, seed=19, distances=(1.0,)), random_rays(200, 6.0),
                           axis_rays(M[list(COPIED)], lo, hi, 32, 23), axis_rays(M[:N_REGULAR], lo, hi, 4, 24), degenerate_rays()])
    assert 600 <= len(rays) <= 1000
    return rays


def input_statistics(lists):
    """(rays with more than 16 pairs, rays with pairs in two or more instances, rays with an equal-t pair)"""
    return (sum(1 for h in lists if len(h) > 16), sum(1 for h in lists if len({x[3] for x in h}) >= 2),
            sum(1 for h in lists if any(a[0] == b[0] for a, b in zip(h, h[1:]))))


@pytest.fixture(scope="module", params=["cube", "quads"])
def multi(request):
    arrays, tris = unit_cube() if request.param == "cube" else stacked_quads_meshes(12, 0.25, flip_every=3)
    M, masks = make_table()
    return dict(name=request.param, scene=Scene(*arrays), tris=tris, mot=mesh_of_triangles(arrays[4]), M=M, masks=masks, rays=make_rays(M, tris),
                W=None, lists=None, cands=None)


def table_context(s, build=None):
    """a context with the fixture's table installed; the brute force (it depends on W alone) is made once and shared"""
    r = context(s["scene"], build)
    r.set_instances(s["M"], s["masks"])
    W, _ = r.instances_readback()
    if s["lists"] is None:
        live = live_of(W)
        assert np.all(live[:N_REGULAR]) and np.all(live[-len(COPIED):]), "every regular transform and every copy is live"
        assert not np.any(live[N_REGULAR:-len(COPIED)][extreme_transforms()[1]]), "singular and non-finite transforms are inert"
        s["cands"] = candidates(s["rays"], W, live, s["tris"])
        s["W"], s["lists"] = W, expected(s["rays"], W, live, s["masks"], s["tris"], s["mot"], cands=s["cands"])[3]
        for h in s["lists"]:
            keys = [(float(t), i, g) for t, _, _, i, g in h]
            assert keys == sorted(keys) and len(set(keys)) == len(keys), "a hit list is strictly ascending in (t, i, g)"
    assert np.array_equal(bits(W), bits(s["W"])), "W does not depend on the builder"
    return r


# ---- 1. bit-exact against the brute force ----
@pytest.mark.parametrize("no_wide", (0, 1))
@pytest.mark.parametrize("build", (AUTO, LBVH))
def test_bit_exact_against_brute_force(native_lib, multi, build, no_wide):
    s = multi
    r = table_context(s, build)
    try:
        # what the inputs reach, from the brute force alone.  The deep lists and the equal-t pairs are the stacked quads' (a cube
        # gives an instance two pairs on most rays; a ray through a quad's diagonal hits both of its triangles at one t)
        deep, shared, ties = input_statistics(s["lists"])
        print("%s: %d rays, %d with > 16 pairs, %d with >= 2 instances, %d with an equal-t pair, longest list %d" % (
            s["name"], len(s["rays"]), deep, shared, ties, max(len(h) for h in s["lists"])))
        assert shared >= 100
        if s["name"] == "quads":
            assert deep >= 100 and ties >= 20
        r.debug_switch("CAP_NO_WIDE8", no_wide)
        check_pages(r, s["rays"], s["lists"], "%s builder %d no_wide8 %d" % (s["name"], build, no_wide))
    finally:
        r.close()


# ---- 2. k = 1 is the closest query ----
def test_k1_is_the_closest_query(native_lib, multi):
    s = multi
    r = table_context(s)
    try:
        r.set_instance_masks((1 << (np.arange(s["scene"].meshes.reshape(-1, 8).shape[0]) % 6)).astype(np.uint8))
        for cull, mask in ((None, None), ("back", None), ("front", 0x33), (None, 0x0F)):
            hits, inst = r.trace_instances(s["rays"], cull=cull, mask=mask)
            for counts in (False, True):
                out = r.trace_instances_multi(s["rays"], 1, counts=counts, cull=cull, mask=mask)
                assert np.array_equal(bits(out[0][:, 0]), bits(hits)) and np.array_equal(out[1][:, 0], inst), (cull, mask, counts)
            if cull is None and mask is None:
                assert (inst != -1).sum() > len(inst) // 4
    finally:
        r.close()


# ---- 3. paging walks every pair once ----
@pytest.mark.parametrize("k,counts", ((1, True), (3, True), (3, False), (16, True)))
def test_paging_walks_every_pair_once(native_lib, multi, k, counts):
    s = multi
    r = table_context(s)
    try:
        check_paging(r, s["rays"], s["lists"], k, counts, s["name"])
    finally:
        r.close()


# ---- 4. ties across a page boundary, by construction: coinciding copies against the flattened scene ----
def test_ties_across_pages_and_the_flattened_scene(native_lib):
    import torch
    arrays, tris = grid_scene(30)
    T = len(tris)
    tr = np.array([[0, 0, 0], [16, 0, 0], [0, 0, 0], [-32, 16, 48], [64, -64, 16], [16, 0, 0], [-64, 64, -64]], f32)  # coinciding copies
    twin = {0: 2, 1: 5}
    rays = np.concatenate([grid_rays(1500, tr), degenerate_rays()])
    rt = torch.as_tensor(rays, device="cuda:0")
    a = context(Scene(*arrays))
    b = context(Scene(*flatten(arrays, tr)))
    try:
        assert a.set_instances(translations(tr)).inert == 0
        W, _ = a.instances_readback()
        assert np.array_equal(W, translations(-tr))

        def same(out, flat, counts, what):
            h, i, f = bits(np.asarray(out[0].cpu())), np.asarray(out[1].cpu()), bits(np.asarray(flat[0].cpu() if counts else flat.cpu()))
            assert np.array_equal(h[..., :3], f[..., :3]), "%s: t, u, v differ from the flattened scene's" % what
            miss = f[..., 3] == MISS
            assert np.array_equal(h[..., 3] == MISS, miss) and np.all(i[miss] == -1), what
            assert np.array_equal(i[~miss].astype(np.int64) * T + h[..., 3][~miss], f[..., 3][~miss].astype(np.int64)), what  # flat id = copy * T + id
            if counts:
                assert np.array_equal(np.asarray(out[2].cpu()), np.asarray(flat[1].cpu())), "%s: counts" % what
            return h, i

        for k in (4, 16):
            same(a.trace_instances_multi(rt, k, counts=True), b.trace_rays_multi(rt, k, counts=True), True, "k %d" % k)
            same(a.trace_instances_multi(rt, k), b.trace_rays_multi(rt, k), False, "k %d pruned" % k)
        assert np.array_equal(a.trace_instances_multi(rt, 0, counts=True)[2].cpu().numpy(), b.trace_rays_multi(rt, 0, counts=True)[1].cpu().numpy())
        # k = 1 pages on both: the same walk; coinciding copies come in ascending instance order, none lost
        seq = [[] for _ in rays]
        pa = pb = None
        for step in range(200):
            oa = a.trace_instances_multi(rt, 1, counts=True, resume=pa)
            ob = b.trace_rays_multi(rt, 1, counts=True, resume=pb)
            pa, pb = (oa[0], oa[1]), ob[0]
            h, i = same(oa, ob, True, "k 1 page %d" % step)
            if np.all(i == -1):
                break
            for j in np.flatnonzero(i[:, 0] != -1):
                seq[j].append((int(h[j, 0, 0]), int(i[j, 0]), int(h[j, 0, 3])))
        assert 2 <= step < 199
        n_twins = 0
        for s in seq:
            assert len(set(s)) == len(s), "a pair appears once"
            for pos, (t, i, g) in enumerate(s):
                if i in twin:  # the coinciding copy's pair follows at the same t, after the lower instance's pairs of that t
                    later = [x for x in s[pos + 1:] if x[0] == t]
                    assert (t, twin[i], g) in later, "the pair of the coinciding copy %d is lost" % twin[i]
                    assert all(x[1] >= i for x in later), "equal t: ascending instance order"
                    n_twins += 1
        assert n_twins > 300, "the copies that coincide are hit"
    finally:
        a.close()
        b.close()


# ---- 5. filters ----
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
        eight = (1 << (np.arange(len(M)) % 8)).astype(np.uint32)
        zero = np.full(len(M), 0xFF, np.uint32)
        zero[::2] = 0
        plain = expected(rays, W, live, None, tris, mot, None, None, None, cands)[3]
        cases = [(None, None, "back", None), (None, None, "front", None), (eight, None, None, 0x15), (eight, mesh_bits, None, None),
                 (eight, mesh_bits, "back", 0x33), (zero, mesh_bits, "front", 0x0F)]
        for im, mm, cull, mask in cases:
            r.set_instances(M, im)
            r.set_instance_masks(mm)
            what = "instance masks %s mesh masks %s cull %s mask %s" % (im is not None, mm is not None, cull, mask)
            lists = expected(rays, W, live, im, tris, mot, mm, cull, mask, cands)[3]
            if im is None and mm is None:
                # a culled near pair must not prune what lies behind it: such rays exist
                hidden = 0
                for full, kept in zip(plain, lists):
                    ks = {(x[3], x[4]) for x in kept}
                    culled = [(float(x[0]), x[3], x[4]) for x in full if (x[3], x[4]) not in ks]
                    hidden += bool(culled and kept and min(culled) < max((float(x[0]), x[3], x[4]) for x in kept))
                print("cull %s: %d of %d rays have a culled pair in front of an accepted one" % (cull, hidden, len(rays)))
                assert hidden >= 50
            check_pages(r, rays, lists, what, ks=(1, 2, 4, 16), cull=cull, mask=mask)
            check_paging(r, rays, lists, 2, False, what, cull=cull, mask=mask)
            check_paging(r, rays, lists, 4, True, what, cull=cull, mask=mask)
    finally:
        r.close()


# ---- 6. objects ----
def test_objects(native_lib):
    parts = [unit_cube()[0], stacked_quads_meshes(12, 0.25, flip_every=3)[0], single_triangle()]
    arrays, ranges = concat(parts)
    tris, tr = scene_triangles(arrays), triangle_ranges(arrays[4], ranges)
    assert tr.tolist() == [[0, 12], [12, 24], [36, 1]]
    mot = mesh_of_triangles(arrays[4])
    M = regular_transforms(30, seed=81, spread=3.0)
    objects = (np.arange(len(M)) % 3).astype(np.uint32)
    masks = np.full(len(M), 0xFF, np.uint32)
    masks[4::9] = 0x0F
    rays = []
    for k, (f, n) in enumerate(tr):
        lo, hi = tris[f:f + n].reshape(-1, 3).min(0), tris[f:f + n].reshape(-1, 3).max(0)
        rays.append(aimed_rays(M[objects == k], lo, hi, 10, seed=82 + k, distances=(1.0, 100.0)))
    rays = np.concatenate(rays + [random_rays(200, 5.0, seed=85), degenerate_rays()])
    r = context(Scene(*arrays))
    try:
        assert r.set_objects(ranges).count == 3
        assert r.set_instances(M, masks, objects=objects).inert == 0
        W, _ = r.instances_readback()
        live = live_of(W)
        cands = object_candidates(rays, W, live, objects, tris, tr)
        rec, inst, _, lists = object_expected(rays, W, live, masks, objects, tris, tr, mot, cands=cands)
        objs_hit = {int(objects[x[3]]) for h in lists for x in h}
        assert objs_hit == {0, 1, 2} and sum(1 for h in lists if any(objects[x[3]] == 2 for x in h)) >= 50, "every object is hit, the one without a node too"
        assert sum(1 for h in lists if len(h) > 4) >= 30, "some lists overflow a page of four"
        for h in lists:
            assert all(tr[objects[i]][0] <= g < tr[objects[i]].sum() for _, _, _, i, g in h)
        check_pages(r, rays, lists, "three objects", ks=(1, 4, 16))
        check_paging(r, rays, lists, 3, True, "three objects")
        # a one-object table covering the whole scene gives the bits of no table
        r.set_objects([(0, len(arrays[4]))])
        r.set_instances(M, masks)
        whole = [r.trace_instances_multi(rays, 5, counts=True), r.trace_instances_multi(rays, 16)]
        r.set_objects(None)
        r.set_instances(M, masks)
        none = [r.trace_instances_multi(rays, 5, counts=True), r.trace_instances_multi(rays, 16)]
        for x, y in zip(whole[0] + whole[1], none[0] + none[1]):
            assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
    finally:
        r.close()


# ---- 7. argument and state errors: nothing is written ----
def test_argument_and_state_errors(native_lib, small):
    import torch
    scene, tris, mot, M, rays = small
    rays = rays[:64]
    n, k = len(rays), 4
    dev = torch.device("cuda", 0)
    L = capi.lib()
    r = context(scene)
    try:
        rt = torch.as_tensor(rays, device=dev)
        buf = torch.full((n * k * 4 + 8,), 7.0, device=dev)     # hits, with room to misalign
        ibuf = torch.full((n * k + 8,), 7, dtype=torch.int32, device=dev)
        cbuf = torch.full((n + 8,), 7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        R, H, I, Cn = rt.data_ptr(), buf.data_ptr(), ibuf.data_ptr(), cbuf.data_ptr()

        def call(rays_p=R, nn=n, kk=k, hits=H, inst=I, counts=Cn, flags=0, opt=None):
            return L.cap_trace_instances_multi(r.ctx, rays_p, nn, kk, hits, inst, counts, flags, ctypes.byref(opt) if opt is not None else None)

        def untouched(what):
            r.sync()
            assert torch.all(buf == 7.0) and torch.all(ibuf == 7) and torch.all(cbuf == 7), "%s: something was written" % what

        assert call() == ERR_STATE and b"cap_instances_set" in L.cap_last_error(), "no instance table"
        untouched("no table")
        r.set_instances(M)
        bad = {
            "k > CAP_MULTI_MAX_K": dict(kk=17),
            "k = 0 with hits": dict(kk=0, inst=None),
            "k = 0 with instances": dict(kk=0, hits=None),
            "k = 0 without counts": dict(kk=0, hits=None, inst=None, counts=None),
            "k > 0 without hits": dict(hits=None),
            "k > 0 without instances": dict(inst=None),
            "CAP_MULTI_CONTINUE with k = 0": dict(kk=0, hits=None, inst=None, flags=1),
            "unknown multi flags": dict(flags=2),
            "first hit": dict(opt=capi.TraceOptions(0x04, 0)),
            "both cull flags": dict(opt=capi.TraceOptions(0x30, 0)),
            "unknown ray flags": dict(opt=capi.TraceOptions(0x100, 0)),
            "reserved words": dict(opt=capi.TraceOptions(0, 0, (ctypes.c_uint32 * 2)(0, 1))),
            "instance_mask > 0xFF": dict(opt=capi.TraceOptions(0, 0x100)),
            "misaligned rays": dict(rays_p=R + 4, nn=n - 1),
            "misaligned hits": dict(hits=H + 8),
            "misaligned instances": dict(inst=I + 2),
            "misaligned counts": dict(counts=Cn + 1),
            "rays overlap hits": dict(rays_p=H, nn=n),
            "hits overlap instances": dict(inst=H + 16 * (n * k - 1)),
            "instances overlap counts": dict(counts=I + 4 * (n * k - 1)),
            "rays overlap counts": dict(counts=R + 32 * (n - 1)),
            "hits overlap counts": dict(counts=H),
            "n * k beyond the address space": dict(nn=1 << 62),
        }
        for what, kw in bad.items():
            assert call(**kw) == ERR_INVALID_ARG, what
            untouched(what)
        assert call(nn=0) == 0 and call(nn=0, hits=None, inst=None, counts=None) == 0, "n = 0 does nothing"
        untouched("n = 0")
        with pytest.raises(capi.CapError):
            r.trace_instances_multi(rays, 17)
        with pytest.raises(capi.CapError):
            r.trace_instances_multi(rays, 0)
        with pytest.raises(capi.CapError):
            r.trace_instances_multi(rays, 2, resume=np.zeros((n, 2, 4), f32))
        # stale trees after a vertex update until the refit
        r.update_vertices(scene.positions)
        assert call() == ERR_STATE
        untouched("stale")
        r.refit_bvh()
        assert call() == 0
        r.sync()
        assert not torch.all(buf[:n * k * 4] == 7.0) and torch.all(buf[n * k * 4:] == 7.0) and torch.all(ibuf[n * k:] == 7) and torch.all(cbuf[n:] == 7)
        buf.fill_(7.0), ibuf.fill_(7), cbuf.fill_(7)
        torch.cuda.synchronize()
        # set_objects drops the table
        r.set_objects([(0, 6)])
        assert call() == ERR_STATE
        untouched("after set_objects")
    finally:
        r.close()
    r = capi.Renderer(0)
    try:
        r.upload_scene(scene.positions, scene.normals, scene.texcoords, scene.indices, scene.meshes)
        assert L.cap_trace_instances_multi(r.ctx, R, n, k, H, I, Cn, 0, None) == ERR_STATE and b"cap_bvh_build" in L.cap_last_error()
        r.sync()
        assert torch.all(buf == 7.0) and torch.all(ibuf == 7) and torch.all(cbuf == 7)
    finally:
        r.close()


# ---- 8. nothing else moved ----
def cornell_frame(r, with_queries=None):
    w = h = 64
    r.set_resolution(w, h)
    r.set_camera(capi.cornell_camera(w, h))
    r.render(0, 2, 2, capi.RENDER_AOV)
    q = with_queries() if with_queries else None
    r.render(2, 2, 2, capi.RENDER_AOV)
    r.sync()
    return bits(r.readback(capi.BUF_ACCUM_SUM)), bits(r.readback(capi.BUF_GBUFFER_GEO)), q


def test_nothing_else_moved(native_lib, bluenoise, cornell_path):
    import torch
    scene, materials = cornell_scene(cornell_path)
    tris = scene.triangles()
    rng = np.random.default_rng(61)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    o = rng.uniform(0.1, 0.9, (300, 3)) * (hi - lo) + lo
    rays = np.c_[o, np.zeros(300), rng.normal(size=(300, 3)), np.full(300, np.inf)].astype(f32)
    M = regular_transforms(12, seed=62, spread=2.0)
    dev = torch.device("cuda", 0)

    def run(interleave):
        r = context(scene, bluenoise=bluenoise)
        try:
            rt = torch.as_tensor(rays, device=dev)
            torch.cuda.synchronize()
            r.set_instances(M)

            def queries():
                first = r.trace_instances_multi(rt, 4, counts=True, sync=False)
                page = r.trace_instances_multi(rt, 2, sync=False)
                more = r.trace_instances_multi(rt, 2, counts=True, sync=False, resume=page)  # (written over `page`)
                return first, more, r.trace_instances_multi(rt, 16, sync=False), r.trace_instances_multi(rt, 0, counts=True, sync=False)

            frame = cornell_frame(r, queries if interleave else None)
            s = r.stats()
            counters = np.array([s.rays_primary, s.rays_extension, s.rays_shadow], np.int64)
            h, i = r.trace_instances(rays)
            plain = (bits(r.trace_rays(rays)), r.trace_occlusion(rays), bits(r.trace_rays_multi(rays, 4)), bits(r.trace_rays(rays, cull="back")),
                     bits(h), i, r.trace_instances_occlusion(rays))
            if interleave:
                W, _ = r.instances_readback()
                lists = expected(rays, W, live_of(W), None, tris)[3]
                first, more, deep, count = frame[2]
                compare(first, expected_pages(lists, rays, 4), True, "interleaved, first page")
                compare(more, expected_pages(lists, rays, 2, 2), True, "interleaved, second page")
                compare(deep, expected_pages(lists, rays, 16), False, "interleaved, k 16")
                compare(count, expected_pages(lists, rays, 0), True, "interleaved, counts only")
            return frame[:2] + (counters,), plain
        finally:
            r.close()

    (fa, pa), (fb, pb) = run(True), run(False)
    for x, y in zip(fa + pa, fb + pb):
        assert np.array_equal(x, y), "the image, the counters or a plain query changed with multi-hit instanced queries interleaved"
