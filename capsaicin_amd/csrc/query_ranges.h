// query_ranges.h — the address checks every ray-query entry point makes on its caller's device arrays (ctx_query.hip), once.
// Plain host C++ without a HIP header, so that a stand-alone program can run it under the host sanitizers
// (tools/query_ranges_check.py) and cap_debug_query_ranges() can show it to tests/test_query_ranges.py.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace cap
{
// One array of a query call: `stride` bytes per ray from `base` on, `base` a multiple of `align`.  An array the caller left out
// (present == false) is not looked at.
struct QueryRange
{
    const char* name;
    uintptr_t   base;
    uint64_t    stride;
    uint32_t    align;
    bool        present;
};

// In this order: every range aligned; n * stride bytes from base stay inside the address space; no two ranges share a byte (an
// empty range shares none).  false: `msg` names the entry point `what` and the offending range or ranges.
inline bool query_ranges_ok(const char* what, uint64_t n, const QueryRange* r, size_t count, char* msg, size_t msg_size)
{
    for (size_t x = 0; x < count; ++x)
        if (r[x].present && (r[x].base & (r[x].align - 1u)))
            return snprintf(msg, msg_size, "%s: %s is not %u-byte aligned", what, r[x].name, r[x].align), false;
    for (size_t x = 0; x < count; ++x)
        if (r[x].present && r[x].stride && n > (UINTPTR_MAX - r[x].base) / r[x].stride)
            return snprintf(msg, msg_size, "%s: %llu rays x %llu bytes of %s exceed the address space", what, (unsigned long long)n,
                            (unsigned long long)r[x].stride, r[x].name),
                   false;
    for (size_t x = 0; x < count; ++x)
        for (size_t y = x + 1; y < count; ++y)
        {
            const uint64_t xb = r[x].present ? n * r[x].stride : 0, yb = r[y].present ? n * r[y].stride : 0;
            if (xb && yb && r[x].base < r[y].base + yb && r[y].base < r[x].base + xb)
                return snprintf(msg, msg_size, "%s: the %s and %s ranges overlap", what, r[x].name, r[y].name), false;
        }
    return true;
}
}  // namespace cap
