"""The address checks of the ray-query entry points (csrc/query_ranges.h): every caller's array aligned, n * stride bytes inside the
address space, no two arrays sharing a byte -- in that order, an array the caller left out never looked at.  cap_debug_query_ranges()
runs them on made-up addresses; cases() is the table (tools/query_ranges_check.py feeds the same table to a sanitized host build).
No GPU."""
import ctypes as C
import itertools

import pytest

OK, ERR_INVALID_ARG = 0, 1
TOP = 1 << 64  # one past UINTPTR_MAX
N = 5          # rays of the ordinary cases: odd, more than one element
# (bytes per ray, alignment) of the arrays of an entry point with 2, 3 and 4 of them: rays, a hit page (k = 1 and 3), an instance
# page (k = 3), counts
LAYOUTS = {2: [(32, 16), (16, 16)], 3: [(32, 16), (48, 16), (4, 4)], 4: [(32, 16), (48, 16), (12, 4), (4, 4)]}


def disjoint(layout, n=N, start=0x7F0000010000, gap=64):
    """aligned bases, `gap` bytes between one array's end and the next one's start"""
    bases, at = [], start
    for stride, _ in layout:
        bases.append(at)
        at += n * stride + gap
    return bases


def cases():
    """(label, n, bases, strides, aligns, expected code, substrings of the message)"""
    out = []

    def add(label, n, bases, layout, code, *words):
        out.append((label, n, list(bases), [s for s, _ in layout], [a for _, a in layout], code, words))

    for count, layout in LAYOUTS.items():
        tag = "%d ranges: " % count
        base = disjoint(layout)
        add(tag + "aligned and disjoint", N, base, layout, OK)
        for i, (stride, align) in enumerate(layout):
            for off in ((4, 8, 12) if align == 16 else (1, 2, 3)):
                b = list(base)
                b[i] += off
                add(tag + "range %d misaligned by %d" % (i, off), N, b, layout, ERR_INVALID_ARG, "range %d" % i, "%d-byte aligned" % align)
        # end to start, in the order of the list and against it (12 rays: every array's length is a multiple of 16)
        for order in (range(count), reversed(range(count))):
            b, at = [0] * count, 0x7F0000010000
            for i in order:
                b[i] = at
                at += 12 * layout[i][0]
            add(tag + "touching end to start", 12, b, layout, OK)
        # range j begins at the last element of range i
        for i, j in itertools.permutations(range(count), 2):
            b = disjoint(layout, start=0x7F0000010000 + (1 << 20))
            b[i] = 0x7F0000010000
            b[j] = b[i] + (N - 1) * layout[i][0]
            add(tag + "range %d starts in the last element of range %d" % (j, i), N, b, layout, ERR_INVALID_ARG, "range %d" % i, "range %d" % j, "overlap")
            # ... and at its last byte only (where the alignment allows that address)
            if layout[j][1] == 4 and layout[i][0] % 4 == 0:
                b[j] = b[i] + N * layout[i][0] - 4
                add(tag + "range %d starts in the last word of range %d" % (j, i), N, b, layout, ERR_INVALID_ARG, "range %d" % i, "range %d" % j, "overlap")
            # an array the caller left out (stride 0) overlaps nothing, wherever its pointer points
            absent = list(layout)
            absent[j] = (0, layout[j][1])
            add(tag + "absent range %d on top of range %d" % (j, i), N, b, absent, OK)
            b[j] += 1
            add(tag + "absent range %d, misaligned, inside range %d" % (j, i), N, b, absent, OK)
        # n * stride wraps to little or nothing in 64 bits: every stride alone, the other arrays left out
        for i in range(count):
            for stride in (4, 12, 16, 32, 48, 1024):
                alone = [(stride if x == i else 0, a) for x, (_, a) in enumerate(layout)]
                add(tag + "2^62 rays x %d bytes in range %d" % (stride, i), 1 << 62, base, alone, ERR_INVALID_ARG, "range %d" % i, "address space")
            add(tag + "2^62 rays, every range", 1 << 62, base, layout, ERR_INVALID_ARG, "range 0", "address space")
        # at the top of the address space: the last byte may be UINTPTR_MAX, and no further
        for i, (stride, align) in enumerate(layout):
            fits = (TOP - 1 - N * stride) // align * align
            for b_i, code in ((fits, OK), (fits + align, ERR_INVALID_ARG), (TOP - align, ERR_INVALID_ARG)):
                b = list(base)
                b[i] = b_i
                add(tag + "range %d at 2^64 - %d" % (i, TOP - b_i), N, b, layout, code, *(("range %d" % i, "address space") if code else ()))
    return out


CASES = cases()


def run(lib, n, bases, strides, aligns):
    count = len(bases)
    return lib.cap_debug_query_ranges(n, count, (C.c_uint64 * count)(*bases), (C.c_uint64 * count)(*strides), (C.c_uint32 * count)(*aligns))


@pytest.mark.parametrize("count", sorted(LAYOUTS))
def test_table(native_lib, count):
    mine = [c for c in CASES if len(c[2]) == count]
    assert len(mine) > 30
    for label, n, bases, strides, aligns, code, words in mine:
        assert run(native_lib, n, bases, strides, aligns) == code, (label, native_lib.cap_last_error())
        message = native_lib.cap_last_error().decode()
        if code:
            assert message.startswith("cap_debug_query_ranges: ") and all(w in message for w in words), (label, message)


def test_order_of_the_checks(native_lib):
    """alignment before the address space before the overlaps, as the entry points always had it"""
    layout = LAYOUTS[3]
    strides, aligns = [s for s, _ in layout], [a for _, a in layout]
    b = disjoint(layout)
    b[1] = b[0]                  # overlaps range 0 ...
    b[2] = TOP - 4               # ... range 2 wraps ...
    assert run(native_lib, N, b, strides, aligns) == ERR_INVALID_ARG and b"address space" in native_lib.cap_last_error()
    b[0] += 4                    # ... and range 0 is misaligned
    assert run(native_lib, N, b, strides, aligns) == ERR_INVALID_ARG and b"range 0 is not 16-byte aligned" in native_lib.cap_last_error()


def test_bad_arguments(native_lib):
    one = (C.c_uint64 * 1)(64)
    assert native_lib.cap_debug_query_ranges(1, 0, None, None, None) == OK  # no array, nothing to refuse
    assert native_lib.cap_debug_query_ranges(1, 1, None, one, (C.c_uint32 * 1)(4)) == ERR_INVALID_ARG
    assert native_lib.cap_debug_query_ranges(1, 5, one, one, (C.c_uint32 * 1)(4)) == ERR_INVALID_ARG
    assert native_lib.cap_debug_query_ranges(1, 1, one, one, (C.c_uint32 * 1)(12)) == ERR_INVALID_ARG  # not a power of two
