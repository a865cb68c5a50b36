"""The pieces of the small-scene candidate mask that need no device (csrc/cap_exhaustive.h): the two sign flips as bitop3 truth
tables, the carry-chain insertion m = 2 m + inside in the order the kernel walks the list, and the host's rule for which scenes
take it (cap_debug_pair_ids_dense, what upload_fan_records asks)."""
import ctypes as C

import numpy as np

K = 0x80000000


def bitop3(a, b, c, table):
    """v_bitop3_b32: bit i of the result is bit (a_i << 2 | b_i << 1 | c_i) of the table"""
    out = 0
    for i in range(32):
        sel = ((a >> i) & 1) << 2 | ((b >> i) & 1) << 1 | ((c >> i) & 1)
        out |= ((table >> sel) & 1) << i
    return out


def test_truth_tables_over_all_input_bits():
    for sel in range(8):
        a, b, c = (sel >> 2) & 1, (sel >> 1) & 1, sel & 1
        assert (0x6c >> sel) & 1 == b ^ (a & c)          # x ^ (ddn & K)
        assert (0xc6 >> sel) & 1 == b ^ ((a ^ 1) & c)    # x ^ (~ddn & K)


def test_flips_equal_the_plain_expressions():
    rs = np.random.RandomState(7)
    words = [0, K, 0x7fffffff, 0xffffffff, 0x3f800000, 0xbf800000] + [int(v) for v in rs.randint(0, 2 ** 32, 64, dtype=np.uint64)]
    for ddn in words:
        s = ddn & K
        for x in words:
            assert bitop3(ddn, x, K, 0x6c) == x ^ s
            assert bitop3(ddn, x, K, 0xc6) == x ^ (s ^ K)
            # a sign word that is masked already (the any-hit table) goes in unchanged
            assert bitop3(s, x, K, 0x6c) == x ^ s and bitop3(s, x, K, 0xc6) == x ^ (s ^ K)


def carry_chain(inside, words):
    """inside[i]: triangle i's bit; the kernel's walk: last pair first, in a pair the second triangle first, i.e. ids descending.
    One word: v_addc m, -, m, m, bit.  Two words: the low word's carry-out is the high word's carry-in."""
    m = [0] * words
    for i in range(len(inside) - 1, -1, -1):
        carry = int(inside[i])
        for w in range(words):
            t = 2 * m[w] + carry
            m[w], carry = t & 0xffffffff, t >> 32
        assert carry == 0  # at most 32 * words steps: nothing leaves the top
    return m


def test_carry_chain_equals_the_id_indexed_mask():
    rs = np.random.RandomState(11)
    for n in list(range(1, 33)) + list(range(33, 65)):
        words = 1 if n <= 32 else 2
        for pattern in ("random", "random", "ones", "zeros", "ends"):
            if pattern == "random":
                inside = rs.randint(0, 2, n)
            elif pattern == "ones":
                inside = np.ones(n, int)
            elif pattern == "zeros":
                inside = np.zeros(n, int)
            else:
                inside = np.zeros(n, int)
                inside[0] = inside[n - 1] = 1
            want = sum(int(b) << i for i, b in enumerate(inside))
            got = carry_chain(inside, words)
            assert got[0] == want & 0xffffffff
            if words == 2:
                assert got[1] == want >> 32
            else:
                assert want >> 32 == 0


def records(ids):
    r = np.zeros((max(len(ids), 1), 20), np.float32)
    r[:len(ids), 18] = np.uint32(ids).view(np.float32)
    return r


def dense(native_lib, ids, singles, ntri):
    r = records(ids)
    return native_lib.cap_debug_pair_ids_dense(r.ctypes.data_as(C.c_void_p), len(ids), singles, ntri)


def test_pair_ids_dense_predicate(native_lib):
    assert dense(native_lib, [0], 0, 2) == 1
    assert dense(native_lib, [0, 2, 4], 0, 6) == 1
    assert dense(native_lib, list(range(0, 64, 2)), 0, 64) == 1
    # a loose triangle: behind the pairs, between them (the ids after it are odd), in front
    assert dense(native_lib, [0, 2], 1, 5) == 0
    assert dense(native_lib, [0, 3], 1, 5) == 0
    assert dense(native_lib, [1, 3], 1, 5) == 0
    # ids offset although the counts fit; pairs out of order
    assert dense(native_lib, [1, 3], 0, 4) == 0
    assert dense(native_lib, [2, 0], 0, 4) == 0
    assert dense(native_lib, [0, 2], 0, 5) == 0
    # no triangles: nothing to walk
    assert dense(native_lib, [], 0, 0) == 0
    assert native_lib.cap_debug_pair_ids_dense(None, 0, 0, 0) == 0
