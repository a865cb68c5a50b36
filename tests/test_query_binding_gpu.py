"""The plumbing of capi.py's twelve query wrappers on the MI355X: where results live (tensor in, tensors out; numpy in, numpy out;
out= and resume pages written in place and handed back), their shapes, dtypes and tuple arity, which entry point each call reaches
and with which NULL pointers, sync=False on torch's stream, and that every rejected input raises CapError before anything is
launched.  What the records hold is the other query suites' job: here two calls are only ever compared with each other, on their
raw bytes.  Cornell box, three instances (identity, a translation, a mirror), 65 rays and 65 points: 65 crosses one wave."""
import numpy as np
import pytest

from capsaicin_amd import capi

pytestmark = pytest.mark.gpu
N = 65
SENTINEL = 0x7FBADBAD  # a NaN no record holds, and no id or count either
F, I = "float32", "int32"

# wrapper: (input, [(shape of a result behind N, dtype), ...]); the multi wrappers' shapes are behind (N, k), counts come last
SINGLE = {
    "trace_rays": ("rays", [((4,), F)]),
    "trace_occlusion": ("rays", [((), I)]),
    "trace_instances": ("rays", [((4,), F), ((), I)]),
    "trace_instances_occlusion": ("rays", [((), I)]),
    "closest_points": ("points", [((8,), F)]),
    "signed_distance": ("points", [((8,), F), ((), F)]),
    "closest_instances": ("points", [((8,), F), ((), I)]),
    "signed_distance_instances": ("points", [((8,), F), ((), I), ((), F)]),
}
MULTI = {
    "trace_rays_multi": ("rays", [((4,), F)]),
    "trace_instances_multi": ("rays", [((4,), F), ((), I)]),
    "closest_points_multi": ("points", [((8,), F)]),
    "closest_instances_multi": ("points", [((8,), F), ((), I)]),
}
WRAPPERS = {**SINGLE, **MULTI}
WIDTH = {"rays": 8, "points": 4}
PLAIN_AND_EX = {"trace_rays": [dict(cull="back"), dict(mask=1), dict(first_hit=True)], "trace_occlusion": [dict(cull="back"), dict(mask=1)],
                "trace_rays_multi": [dict(cull="back"), dict(mask=1)]}
QUERY_SYMBOLS = ("cap_trace_rays", "cap_trace_occlusion", "cap_trace_rays_multi", "cap_trace_rays_ex", "cap_trace_occlusion_ex",
                 "cap_trace_rays_multi_ex", "cap_trace_instances", "cap_trace_instances_occlusion", "cap_trace_instances_multi",
                 "cap_closest_points", "cap_closest_points_multi", "cap_signed_distance", "cap_closest_instances",
                 "cap_signed_distance_instances", "cap_closest_instances_multi")


def torch_dev():
    import torch
    return torch.device("cuda", 0)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def same(a, b):
    a, b = host(a), host(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def as_tuple(res, parts):
    """the results as a tuple; a wrapper with one result returns it bare, the others a tuple"""
    assert isinstance(res, tuple) == (parts > 1), type(res)
    res = res if isinstance(res, tuple) else (res,)
    assert len(res) == parts
    return res


def check_layout(res, spec, lead, on_device):
    import torch
    for a, (tail, dtype) in zip(res, spec):
        if on_device:
            assert isinstance(a, torch.Tensor) and a.device == torch_dev() and a.dtype == getattr(torch, dtype), (type(a), a.dtype)
        else:
            assert isinstance(a, np.ndarray) and a.dtype == np.dtype(dtype), (type(a), a.dtype)
        assert tuple(a.shape) == lead + tail, (tuple(a.shape), lead + tail)


def multi_spec(name, counts):
    return MULTI[name][1] + ([((), I)] if counts else [])


def multi_lead(n, k, spec, counts):
    """the leading shapes of a multi call's results: (n, k) for the pages, (n,) for the counts"""
    return [(n, k)] * (len(spec) - counts) + [(n,)] * counts


def check_multi(res, name, k, counts, on_device):
    spec = multi_spec(name, counts)
    res = as_tuple(res, len(spec))
    for a, s, lead in zip(res, spec, multi_lead(N, k, spec, counts)):
        check_layout((a,), (s,), lead, on_device)
    return res


def sentinel(shape, dtype):
    import torch
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=torch_dev()).view(getattr(torch, dtype))


def untouched(*tensors):
    import torch
    return all(bool((t.view(torch.int32) == SENTINEL).all()) for t in tensors)


def make_renderer(path, stream=None):
    r = capi.Renderer(0, stream)
    geo = capi.Geometry(path)
    r.upload_geometry(geo)
    r.build_bvh()
    r.build_pseudonormals()  # (defined for the box's open front too: closed == 0 only says what the sign means)
    t = np.zeros((3, 3, 4), np.float32)
    t[:, 0, 0] = t[:, 1, 1] = t[:, 2, 2] = 1.0
    t[1, 0, 3] = 2.5  # a translation
    t[2, 0, 0], t[2, 0, 3] = -1.0, -2.5  # a mirror
    r.set_instances(t)
    return r, geo


@pytest.fixture(scope="module")
def scene(native_lib, cornell_path):
    """(renderer, {"rays": (N, 8), "points": (N, 4)} numpy, the same as tensors)"""
    import torch
    r, geo = make_renderer(cornell_path)
    P = geo.positions.reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    rng = np.random.default_rng(65)
    rays = np.zeros((N, 8), np.float32)
    rays[:, 0:3] = rng.uniform(lo + 0.1, hi - 0.1, (N, 3))
    d = rng.normal(size=(N, 3))
    rays[:, 4:7], rays[:, 7] = d / np.linalg.norm(d, axis=1, keepdims=True), np.inf
    points = np.zeros((N, 4), np.float32)
    points[:, 0:3], points[:, 3] = rng.uniform(lo + 0.1, hi - 0.1, (N, 3)), np.inf
    x = {"rays": rays, "points": points}
    for a in x.values():
        a.setflags(write=False)
    yield r, x, {k: torch.as_tensor(v.copy(), device=torch_dev()) for k, v in x.items()}
    r.close()


@pytest.fixture
def calls(monkeypatch, native_lib):
    """every query symbol of the library replaced by a recorder that forwards: the list of (symbol, arguments behind the context)"""
    seen = []
    for name in QUERY_SYMBOLS:
        def recorder(*a, _name=name, _fn=getattr(native_lib, name)):
            seen.append((_name, a[1:]))
            return _fn(*a)
        monkeypatch.setattr(native_lib, name, recorder)
    return seen


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. tensor in, tensors out; numpy in, numpy out, the same bytes
@pytest.mark.parametrize("name", SINGLE)
def test_single_tensor_and_numpy_agree(scene, name):
    r, x, t = scene
    kind, spec = SINGLE[name]
    dev = as_tuple(getattr(r, name)(t[kind]), len(spec))
    check_layout(dev, spec, (N,), True)
    cpu = as_tuple(getattr(r, name)(x[kind]), len(spec))
    check_layout(cpu, spec, (N,), False)
    assert all(same(a, b) for a, b in zip(dev, cpu))


@pytest.mark.parametrize("counts", [False, True])
@pytest.mark.parametrize("name", MULTI)
def test_multi_tensor_and_numpy_agree(scene, name, counts):
    r, x, t = scene
    kind = MULTI[name][0]
    dev = check_multi(getattr(r, name)(t[kind], 2, counts=counts), name, 2, counts, True)
    cpu = check_multi(getattr(r, name)(x[kind], 2, counts=counts), name, 2, counts, False)
    assert all(same(a, b) for a, b in zip(dev, cpu))


@pytest.mark.parametrize("name", MULTI)
def test_multi_counts_only(scene, name):
    """k = 0: pages of no slots, the counts those of a call with slots"""
    r, x, t = scene
    kind = MULTI[name][0]
    dev = check_multi(getattr(r, name)(t[kind], 0, counts=True), name, 0, True, True)
    cpu = check_multi(getattr(r, name)(x[kind], 0, counts=True), name, 0, True, False)
    assert same(dev[-1], cpu[-1])
    assert same(dev[-1], getattr(r, name)(t[kind], 2, counts=True)[-1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. out=
@pytest.mark.parametrize("name", SINGLE)
def test_out_tensor_is_written_in_place(scene, name):
    r, x, t = scene
    kind, spec = SINGLE[name]
    want = as_tuple(getattr(r, name)(t[kind]), len(spec))
    tail, dtype = spec[0]
    buf = sentinel((N + 8,) + tail, dtype)
    out = buf[4:N + 4]  # (16-byte aligned for the (N,) int32 outputs too)
    res = as_tuple(getattr(r, name)(t[kind], out=out), len(spec))
    assert res[0].data_ptr() == out.data_ptr() and tuple(res[0].shape) == (N,) + tail
    assert all(same(a, b) for a, b in zip(res, want))
    assert same(out, want[0]) and untouched(buf[:4], buf[N + 4:])


@pytest.mark.parametrize("numpy_input", [False, True])
@pytest.mark.parametrize("name", SINGLE)
def test_out_numpy_is_filled_and_returned(scene, name, numpy_input):
    r, x, t = scene
    kind, spec = SINGLE[name]
    want = as_tuple(getattr(r, name)(x[kind]), len(spec))
    tail, dtype = spec[0]
    out = np.full((N,) + tail, 7, np.dtype(dtype))
    res = as_tuple(getattr(r, name)((x if numpy_input else t)[kind], out=out), len(spec))
    assert res[0] is out
    check_layout(res, spec, (N,), False)
    assert all(same(a, b) for a, b in zip(res, want))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. paging
@pytest.mark.parametrize("name", MULTI)
def test_paging(scene, name):
    """two pages of k = 2 are the first four slots of one k = 4 call; a tensor page is written over and returned, a numpy page is
    filled and returned"""
    import torch
    r, x, t = scene
    kind = MULTI[name][0]
    call = getattr(r, name)
    pages = len(MULTI[name][1])
    full = as_tuple(call(t[kind], 4), pages)
    first = as_tuple(call(t[kind], 2), pages)
    assert all(same(a, b[:, 0:2].contiguous()) for a, b in zip(first, full))
    keep = [a.cpu().numpy().copy() for a in first]

    def resume_of(p):
        return tuple(p) if pages > 1 else p[0]

    second = as_tuple(call(t[kind], 2, resume=resume_of(first)), pages)
    assert all(a is b for a, b in zip(second, first))
    assert all(same(a, b[:, 2:4].contiguous()) for a, b in zip(second, full))
    for inputs in (t, x):  # numpy pages: with tensors and with numpy in
        mine = [a.copy() for a in keep]
        res = check_multi(call(inputs[kind], 2, resume=resume_of(mine)), name, 2, False, False)
        assert all(a is b for a, b in zip(res, mine))
        assert all(same(a, b[:, 2:4].contiguous()) for a, b in zip(res, full))
    # counts ride along behind the pages: those of the hits after the cursor
    mine = [a.copy() for a in keep]
    res = check_multi(call(t[kind], 2, counts=True, resume=resume_of(mine)), name, 2, True, False)
    assert all(a is b for a, b in zip(res, mine))
    both = [torch.as_tensor(a, device=torch_dev()) for a in keep]
    res_t = check_multi(call(t[kind], 2, counts=True, resume=resume_of(both)), name, 2, True, True)
    assert all(a is b for a, b in zip(res_t, both)) and all(same(a, b) for a, b in zip(res_t, res))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. which entry point, with which pointers
def value(a):
    """an argument as the recorder saw it: None for NULL, an int, or "ref" for byref(options) / a pointer"""
    return a if a is None or isinstance(a, int) else "ref"


@pytest.mark.parametrize("name", WRAPPERS)
def test_symbol_and_pointers(scene, calls, name):
    r, x, t = scene
    kind = WRAPPERS[name][0]
    multi = name in MULTI
    call = (lambda **kw: getattr(r, name)(t[kind], 2, **kw)) if multi else (lambda **kw: getattr(r, name)(t[kind], **kw))

    def one():
        assert len(calls) == 1, [c[0] for c in calls]
        return calls.pop()

    call()
    symbol, args = one()
    assert symbol == "cap_" + name
    if name in PLAIN_AND_EX:  # the plain entry point: no options argument; the single ones take flags 0 in its place
        assert len(args) == (6 if multi else 4) and value(args[-1]) == 0
        for kw in PLAIN_AND_EX[name]:
            call(**kw)
            symbol, args = one()
            assert symbol == "cap_" + name + "_ex" and value(args[-1]) == "ref", (kw, symbol)
    else:
        assert value(args[-1]) is None  # options: NULL
        call(mask=1)
        symbol, args = one()
        assert symbol == "cap_" + name and value(args[-1]) == "ref"
    if not multi:
        return
    # (input, n, k, page[, instances], counts, flags[, options])
    pages = len(MULTI[name][1])
    call()
    _, args = one()
    assert [value(a) for a in args[1:3]] == [N, 2] and all(value(a) == "ref" for a in args[3:3 + pages])
    assert value(args[3 + pages]) is None and value(args[4 + pages]) == 0
    call(counts=True)
    _, args = one()
    assert value(args[3 + pages]) == "ref" and value(args[4 + pages]) == 0
    first = call()
    one()
    call(resume=first)
    _, args = one()
    assert value(args[4 + pages]) == capi.Renderer.MULTI_CONTINUE and all(value(a) == "ref" for a in args[3:3 + pages])
    getattr(r, name)(t[kind], 0, counts=True)
    _, args = one()
    assert value(args[2]) == 0 and all(value(a) is None for a in args[3:3 + pages]) and value(args[3 + pages]) == "ref"


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. sync=False on a renderer created on torch's stream
@pytest.fixture(scope="module")
def stream_scene(native_lib, cornell_path, scene):
    import torch
    stream = torch.cuda.Stream(torch_dev())  # (a stream of its own: the null stream's handle is 0, which cap_ctx_create reads as "make one")
    with torch.cuda.stream(stream):
        r, _ = make_renderer(cornell_path, stream.cuda_stream)
    yield r, stream
    r.close()


@pytest.mark.parametrize("name", WRAPPERS)
def test_sync_false_on_torch_stream(scene, stream_scene, name):
    import torch
    _, x, _ = scene
    r, stream = stream_scene
    kind, spec = WRAPPERS[name]
    k = (2,) if name in MULTI else ()
    with torch.cuda.stream(stream):
        t = torch.as_tensor(x[kind].copy(), device=torch_dev())
        res = as_tuple(getattr(r, name)(t, *k, sync=False), len(spec))
        check_layout(res, spec, (N,) + k, True)
        stream.synchronize()
        got = [a.cpu().numpy() for a in res]
        want = as_tuple(getattr(r, name)(t, *k, sync=True), len(spec))
        assert all(same(a, b) for a, b in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. rejections: CapError, and nothing written
def bad_inputs(t, kind):
    import torch
    w = WIDTH[kind]
    good = t[kind]
    return {
        "float64": good.double(),
        "wrong width": torch.zeros((N, 12 - w), dtype=torch.float32, device=torch_dev()),  # (N, 4) rays, (N, 8) points
        "not contiguous": torch.cat([good, good], 1)[:, :w],
        "on the CPU": good.cpu(),
    }


@pytest.mark.parametrize("what", ["float64", "wrong width", "not contiguous", "on the CPU"])
@pytest.mark.parametrize("name", WRAPPERS)
def test_rejects_bad_input(scene, calls, name, what):
    r, x, t = scene
    kind, spec = WRAPPERS[name]
    bad = bad_inputs(t, kind)[what]
    assert tuple(bad.shape) == ((N, 12 - WIDTH[kind]) if what == "wrong width" else (N, WIDTH[kind]))
    if name in MULTI:
        outs = [sentinel((N, 2) + tail, dtype) for tail, dtype in spec]
        with pytest.raises(capi.CapError):
            getattr(r, name)(bad, 2, resume=tuple(outs) if len(outs) > 1 else outs[0])
    else:
        outs = [sentinel((N,) + spec[0][0], spec[0][1])]
        with pytest.raises(capi.CapError):
            getattr(r, name)(bad, out=outs[0])
    assert untouched(*outs) and not calls


@pytest.mark.parametrize("what", ["shape", "dtype"])
@pytest.mark.parametrize("name", SINGLE)
def test_rejects_bad_out(scene, calls, name, what):
    r, x, t = scene
    kind, spec = SINGLE[name]
    tail, dtype = spec[0]
    out = sentinel((N + 1,) + tail, dtype) if what == "shape" else sentinel((N,) + tail, I if dtype == F else F)
    with pytest.raises(capi.CapError):
        getattr(r, name)(t[kind], out=out)
    assert untouched(out) and not calls


@pytest.mark.parametrize("name", MULTI)
def test_rejects_bad_k(scene, calls, name):
    r, x, t = scene
    kind, spec = MULTI[name]
    call = getattr(r, name)

    def resume_of(k):
        p = [sentinel((N, k) + tail, dtype) for tail, dtype in spec]
        return p, (tuple(p) if len(p) > 1 else p[0])

    with pytest.raises(capi.CapError):
        call(t[kind], 17)
    pages, resume = resume_of(17)
    with pytest.raises(capi.CapError):
        call(t[kind], 17, resume=resume)
    assert untouched(*pages)
    with pytest.raises(capi.CapError):
        call(t[kind], 0)  # k = 0 without counts
    with pytest.raises(capi.CapError):
        call(t[kind], 0, counts=True, resume=resume_of(0)[1])  # k = 0 with resume
    assert not calls


@pytest.mark.parametrize("name", MULTI)
def test_rejects_tensor_resume_of_the_wrong_shape(scene, calls, name):
    r, x, t = scene
    kind, spec = MULTI[name]
    for wrong in range(len(spec)):
        pages = [sentinel((N, 3 if j == wrong else 2) + tail, dtype) for j, (tail, dtype) in enumerate(spec)]
        with pytest.raises(capi.CapError):
            getattr(r, name)(t[kind], 2, resume=tuple(pages) if len(pages) > 1 else pages[0])
        assert untouched(*pages)
    assert not calls


@pytest.mark.parametrize("numpy_input", [False, True])
@pytest.mark.parametrize("name", MULTI)
def test_rejects_numpy_resume_of_the_wrong_size(scene, calls, name, numpy_input):
    r, x, t = scene
    kind, spec = MULTI[name]
    for wrong in range(len(spec)):
        pages = [np.full((N, 3 if j == wrong else 2) + tail, 7, np.dtype(dtype)) for j, (tail, dtype) in enumerate(spec)]
        with pytest.raises(capi.CapError):
            getattr(r, name)((x if numpy_input else t)[kind], 2, resume=tuple(pages) if len(pages) > 1 else pages[0])
        assert all((p == 7).all() for p in pages)
    assert not calls


@pytest.mark.parametrize("name", ["trace_instances_multi", "closest_instances_multi"])
def test_rejects_resume_that_is_no_pair(scene, calls, name):
    r, x, t = scene
    kind, spec = MULTI[name]
    pages = [sentinel((N, 2) + tail, dtype) for tail, dtype in spec]
    for resume in (pages[0], (pages[0],), (pages[0], pages[1], pages[1])):
        with pytest.raises(capi.CapError):
            getattr(r, name)(t[kind], 2, resume=resume)
    assert untouched(*pages) and not calls
