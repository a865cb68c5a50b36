"""Render tests for the shading-kernel instantiations that no other test launches (small_scene.hip launch_trace_shade, kernels.hip
launch_shade): the fused small-scene kernels WITHOUT the scene in LDS -- forced exhaustive traversal of a scene just over
kExhaustiveMax = 64 triangles -- for the EXT model (bounce 0 and bounce >= 1) and for G-buffer feedback, and the stand-alone bounce-0
shade stage of the EXT model (tree path with the fused packet-walk stage switched off).  Smallest shapes that select them: 16 x 16
pixels, 1 spp, 2 bounces; every plane and ray counter bit for bit against the CPU oracle, like tests/test_parity_gpu.py."""
import numpy as np
import pytest

from capsaicin_amd import capi
from test_ext_gpu import cornell_with_materials

pytestmark = pytest.mark.gpu

W = H = 16
DEPTH = 2
PLANES = (("gbuffer_geo", capi.BUF_GBUFFER_GEO), ("direct", capi.BUF_DIRECT), ("albedo", capi.BUF_ALBEDO),
          ("normal_depth", capi.BUF_NORMAL_DEPTH), ("indirect", capi.BUF_INDIRECT), ("combined", capi.BUF_COMBINED))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ocam_of(O, cam):
    return O.make_camera(tuple(cam.position), tuple(cam.forward), tuple(cam.right), tuple(cam.up), cam.sensor_size[0], cam.sensor_size[1],
                         cam.focal_length)


@pytest.fixture(scope="module")
def box66(native_lib, tmp_path_factory):
    """The Cornell box (32 triangles), a second copy of it scaled by 2 about its centre around it (no face coplanar with the first
    box's), and a third copy of the floor scaled by 3: 66 triangles in 17 meshes, with the box's materials."""
    geo, mats = cornell_with_materials(tmp_path_factory.mktemp("box66"))
    pos = geo.positions.reshape(-1, 3)
    centre = 0.5 * (pos.min(0) + pos.max(0))
    parts = [(range(len(geo.meshes)), 1.0), (range(len(geo.meshes)), 2.0), ([0], 3.0)]
    P, N, T, I, M, mat = [], [], [], [], [], []
    for which, scale in parts:
        for k in which:
            nv, v0, ni, i0 = (int(x) for x in geo.meshes[k][:4])
            M.append([nv, sum(len(p) for p in P), ni, sum(len(i) for i in I), len(M), int(geo.meshes[k][5]), 0, 0])
            P.append(((pos[v0:v0 + nv] - centre) * np.float32(scale) + centre).astype(np.float32))
            N.append(geo.normals.reshape(-1, 3)[v0:v0 + nv])
            T.append(geo.texcoords.reshape(-1, 2)[v0:v0 + nv])
            I.append(geo.indices[i0:i0 + ni])
            mat.append(mats[k])
    arrays = (np.concatenate(P), np.concatenate(N), np.concatenate(T), np.concatenate(I), np.array(M, np.uint32))
    assert arrays[3].size // 3 == 66
    return arrays, np.array(mat, np.float32)


def renderer(box66, bluenoise):
    arrays, mats = box66
    r = capi.Renderer(0)
    r.upload_scene(*arrays)
    r.upload_materials(mats)
    r.upload_bluenoise(bluenoise)
    assert r.build_bvh().triangle_count == 66
    r.set_resolution(W, H)
    return r


def check_planes(r, ref, what, planes=PLANES):
    for name, kind in planes:
        nbad = int((bits(r.readback(kind)) != bits(ref[name])).any(-1).sum())
        assert nbad == 0, "%s %s: %d pixels differ" % (what, name, nbad)
    s = r.stats()
    assert (s.rays_primary, s.rays_extension, s.rays_shadow) == ref["rays"] and s.guard_shade == 0 and s.guard_trace_any == 0 and s.guard_append == 0


@pytest.mark.parametrize("traversal,no_fuse", [(2, 0), (1, 1)])
def test_ext_model_over_64_triangles(box66, bluenoise, traversal, no_fuse):
    """traversal 2: k_trace_shade<true, true, false, false, false> and <false, true, false, false, false>.
    traversal 1 without the fused bounce-0 stage: k_shade<true, true, false> (and <false, true, false>)."""
    from oracle import cap_oracle as O
    arrays, mats = box66
    r = renderer(box66, bluenoise)
    cam = capi.cornell_camera(W, H)
    r.set_camera(cam)
    r.set_traversal(traversal)
    if no_fuse:
        r.debug_switch("CAP_NO_PRIMARY_FUSE", 1)
    sc = O.Scene(*arrays, materials=mats)
    for frame in (0, 5):
        ref = sc.render_frame(ocam_of(O, cam), bluenoise, W, H, frame, DEPTH, flags=O.FLAG_EXT_MATERIALS)
        assert ref["rays"][1] > 0 and ref["rays"][2] > 0  # the frame has bounces and next-event rays
        r.accum_reset()
        r.stats_reset()
        r.render(frame, 1, DEPTH, capi.RENDER_AOV | capi.RENDER_EXT_MATERIALS)
        check_planes(r, ref, "traversal %d frame %d" % (traversal, frame))
    r.close()


def test_feedback_over_64_triangles(box66, bluenoise):
    """k_trace_shade<false, false, true, false, false>: the reference model with G-buffer feedback, forced exhaustive traversal, scene
    not in LDS.  The loop of tests/test_post_gpu.py test_gbuffer_feedback_parity: render and reconstruction chain feed each other."""
    from oracle import cap_oracle as O
    arrays, _ = box66
    r = renderer(box66, bluenoise)
    r.set_traversal(2)
    sc = O.Scene(*arrays)
    chain = O.PostChain(W, H)
    gs, os_ = capi.PostSettings(), O.PostSettings()
    cam = capi.cornell_camera(W, H)
    prev_nd = np.zeros((H, W, 4), np.float32)
    hist = np.zeros((H, W, 4), np.float32)
    reused = False
    for f in range(3):
        r.set_camera(cam)
        r.set_prev_camera(cam)
        r.stats_reset()
        r.render(f, 1, DEPTH, capi.RENDER_AOV | capi.RENDER_GBUFFER_FEEDBACK)
        ref = sc.render_frame(ocam_of(O, cam), bluenoise, W, H, f, DEPTH, threads=4, feedback=(ocam_of(O, cam), prev_nd, hist))
        plain = sc.render_frame(ocam_of(O, cam), bluenoise, W, H, f, DEPTH, threads=4)
        check_planes(r, ref, "feedback frame %d" % f, PLANES[1:5])
        reused |= ref["rays"][1] < plain["rays"][1]  # paths end early at vertices the last frame saw
        r.post_frame(gs, f, cam)
        want = chain.frame(os_, f, ocam_of(O, cam), ocam_of(O, cam), ref)
        assert np.array_equal(bits(r.post_readback()), bits(want)), "frame %d chain output" % f
        prev_nd, hist = ref["normal_depth"], want
    assert reused
    r.close()
