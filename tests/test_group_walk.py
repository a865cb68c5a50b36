"""head_chunk() (cap_device.h): the head kernels deal bounce 0's chunk indices out so that the frame slots of one jitter group visit a
64-pixel group back to back, band after band.  cap_debug_head_chunk() runs that function on the host; here the mapping is held to what
the kernels rely on, for cps = 64-pixel groups per slot, m = slots per jitter group, several group counts and several permutations of
the slots:
  * it is a bijection of [0, cps * n_slots) onto (slot, 64-pixel group) -- every pair exactly once, nothing out of range;
  * it is the walk it is documented to be: band = c // (m cps), r = c % (m cps), group64 = r // m, slot = order[band m + r % m];
  * the class of a path stays chunk_class(c) of the dealt index, so every class receives at most ceil(chunks / 64) chunks whatever the
    mapping says a chunk means (the static capacity of the sub-queues).
No GPU."""

import numpy as np
import pytest

CPS = (1, 2, 63, 64, 65, 100)
MS = (1, 2, 4, 8)
GROUPS = (1, 2, 3, 8)


def head_chunk(lib, cps, m, order, c):
    order = np.ascontiguousarray(order, np.uint8)
    c = np.ascontiguousarray(c, np.uint32)
    slot, g64 = np.empty_like(c), np.empty_like(c)
    fn = lib.cap_debug_head_chunk  # (declared by capi: every argument a plain integer or address)
    assert fn(cps, m, order.ctypes.data, order.size, c.ctypes.data, c.size, slot.ctypes.data, g64.ctypes.data) == 0
    return slot, g64


def orders(n_slots, m, seed):
    """The identity, the order a 64-frame batch has (group g = slots g, g + groups, ...), and random permutations."""
    groups = n_slots // m
    rs = np.random.RandomState(seed)
    yield np.arange(n_slots)
    yield np.array([g + k * groups for g in range(groups) for k in range(m)])
    for _ in range(3):
        yield rs.permutation(n_slots)


def chunk_class(c):
    return (c + (c >> 6)) & 63


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("groups", GROUPS)
def test_bijection_formula_and_classes(native_lib, m, groups):
    n_slots = m * groups
    for cps in CPS:
        chunks = cps * n_slots
        c = np.arange(chunks, dtype=np.uint32)
        for order in orders(n_slots, m, 1000 * m + 10 * groups + cps):
            slot, g64 = head_chunk(native_lib, cps, m, order, c)
            assert slot.max() < n_slots and g64.max() < cps
            flat = slot.astype(np.int64) * cps + g64  # the slot-major chunk index of what c stands for
            assert flat.max() < chunks  # no index >= cps * n_slots
            assert np.array_equal(np.sort(flat), np.arange(chunks))  # every (slot, 64-pixel group) exactly once
            band, r = np.divmod(c.astype(np.int64), m * cps)
            assert np.array_equal(g64, r // m) and np.array_equal(slot, order[band * m + r % m])
            # the m members of a 64-pixel group are m consecutive indices, and a band holds one group of slots
            assert np.array_equal(g64.reshape(-1, m), np.repeat(g64[::m], m).reshape(-1, m))
            # classes: the dealt index alone decides, so the count per class is that of the identity queue
            per_class = np.bincount(chunk_class(c), minlength=64)
            assert per_class.max() <= (chunks + 63) // 64


def test_m1_identity_is_slot_major(native_lib):
    for cps in CPS:
        for n_slots in (1, 5, 9, 64):
            c = np.arange(cps * n_slots, dtype=np.uint32)
            slot, g64 = head_chunk(native_lib, cps, 1, np.arange(n_slots), c)
            assert np.array_equal(slot, c // cps) and np.array_equal(g64, c % cps)


def test_headline_shape(native_lib):
    """1920 x 1080, 64 slots in 8 groups of 8: cps = 32 400; the ends of every band and random indices."""
    cps, m, n_slots = 32400, 8, 64
    order = np.array([g + 8 * k for g in range(8) for k in range(8)])
    rs = np.random.RandomState(7)
    edges = np.concatenate([np.arange(b * m * cps - 70, b * m * cps + 70) for b in range(1, 8)] + [np.arange(140), np.arange(cps * n_slots - 140, cps * n_slots)])
    c = np.concatenate([edges, rs.randint(0, cps * n_slots, 1_000_000)]).astype(np.uint32)
    slot, g64 = head_chunk(native_lib, cps, m, order, c)
    band, r = np.divmod(c.astype(np.int64), m * cps)
    assert np.array_equal(g64, r // m) and np.array_equal(slot, order[band * m + r % m])
    assert np.array_equal(slot % 8, band)  # a band is one jitter group: slots g, g + 8, ...


def test_largest_queue(native_lib):
    """cps * n_slots = 2^26, the most a path id holds: the two divisions stay exact at the top of the range."""
    cps, m, n_slots = 1 << 20, 8, 64
    order = np.arange(64)
    top = 1 << 26
    rs = np.random.RandomState(11)
    c = np.concatenate([np.arange(top - 4096, top), np.arange(4096), rs.randint(0, top, 1_000_000)]).astype(np.uint32)
    slot, g64 = head_chunk(native_lib, cps, m, order, c)
    band, r = np.divmod(c.astype(np.int64), m * cps)
    assert np.array_equal(g64, r // m) and np.array_equal(slot, order[band * m + r % m])


def test_bad_arguments(native_lib):
    fn = native_lib.cap_debug_head_chunk
    o, c = np.arange(64, dtype=np.uint8), np.zeros(1, np.uint32)
    out = np.zeros(2, np.uint32)
    good = (4, 2, o.ctypes.data, 8, c.ctypes.data, 1, out.ctypes.data, out.ctypes.data + 4)
    assert fn(*good) == 0
    for k, bad in ((0, 0), (1, 0), (1, 3), (2, None), (3, 65), (4, None), (6, None), (7, None)):
        args = list(good)
        args[k] = bad
        assert fn(*args) != 0
    assert fn((1 << 20) + 1, 8, o.ctypes.data, 64, c.ctypes.data, 1, out.ctypes.data, out.ctypes.data + 4) != 0
