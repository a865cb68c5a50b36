"""tile_div() (cap_device.h): the small-scene kernels of bounce >= 1 divide a path's global tile index by tiles_x with a host-computed
multiplier and shift instead of the run-time division.  The form must be exact for every index a path id can hold (26 bits).
cap_debug_tile_divmod() computes quotient and remainder by that form on the host; here it is compared with // and % for every
tiles_x from 1 to 2048 at the neighbours n = k d - 1, k d, k d + 1 of every multiple below 2^26, at n = 2^26 - 1, and at a few million
random n.  No GPU."""
import ctypes as C

import numpy as np

LIMIT = 1 << 26


def divmod_by_form(lib, d, n):
    n = np.ascontiguousarray(n, np.uint32)
    q, r = np.empty_like(n), np.empty_like(n)
    fn = lib.cap_debug_tile_divmod
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    assert fn(d, n.ctypes.data, n.size, q.ctypes.data, r.ctypes.data) == 0
    return q, r


def check(lib, d, n):
    q, r = divmod_by_form(lib, d, n)
    wq, wr = np.divmod(n, np.uint32(d))  # // and % in one pass
    if not (np.array_equal(q, wq) and np.array_equal(r, wr)):
        b = np.flatnonzero((q != wq) | (r != wr))[0]
        raise AssertionError("tiles_x %d: n = %d gives (%d, %d), // and %% give (%d, %d)" % (d, n[b], q[b], r[b], wq[b], wr[b]))
    return n.size


def neighbours(d):
    """k d - 1, k d, k d + 1 for every k with k d < 2^26, and 2^26 - 1 (for d <= 3 that is every n below 2^26, taken once)."""
    if d <= 3:
        return np.arange(LIMIT, dtype=np.uint32)
    m = np.arange(0, LIMIT, d, dtype=np.uint32)
    n = np.empty(3 * m.size, np.uint32)  # n[0] = 0 - 1 is replaced by 2^26 - 1
    np.subtract(m, 1, out=n[:m.size])
    n[0] = LIMIT - 1
    n[m.size:2 * m.size] = m
    np.add(m, 1, out=n[2 * m.size:])
    return n[:-1] if n[-1] >= LIMIT else n


def test_neighbours_of_every_multiple(native_lib):
    # 1.4e9 dividends: numpy and the library both release the interpreter lock, so a few threads share the divisors
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as pool:
        total = sum(pool.map(lambda d: check(native_lib, d, neighbours(d)), range(1, 2049)))
    assert total > 1_400_000_000  # 3 * 2^26 * (1/4 + ... + 1/2048) + 3 * 2^26


def test_random_dividends(native_lib):
    rs = np.random.RandomState(98)
    n = rs.randint(0, LIMIT, 4_000_000).astype(np.uint32)
    for d in (1, 2, 3, 7, 13, 25, 240, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 4096):
        check(native_lib, d, n)
    for d in rs.randint(1, 2049, 2048):  # every call a fresh dividend set
        check(native_lib, int(d), rs.randint(0, LIMIT, 4096).astype(np.uint32))


def test_bad_arguments(native_lib):
    n = np.zeros(1, np.uint32)
    fn = native_lib.cap_debug_tile_divmod
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    assert fn(0, n.ctypes.data, 1, n.ctypes.data, n.ctypes.data) != 0
    assert fn(5, None, 1, n.ctypes.data, n.ctypes.data) != 0
