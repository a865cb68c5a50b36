// Stand-alone driver of csrc/query_ranges.h for the host sanitizers (built and fed by tools/query_ranges_check.py).
// stdin, one case per line:  n count base[count] stride[count] align[count]   (decimal; stride 0 = the array is left out)
// stdout, one line per case:  0  or  1 <message>
#include <cinttypes>
#include <cstdio>

#include "../capsaicin_amd/csrc/query_ranges.h"

int main()
{
    static const char* const names[4] = {"range 0", "range 1", "range 2", "range 3"};
    uint64_t n;
    unsigned count;
    while (scanf("%" SCNu64 " %u", &n, &count) == 2)
    {
        if (count > 4) return 2;
        uint64_t base[4], stride[4];
        uint32_t align[4];
        for (unsigned i = 0; i < count; ++i)
            if (scanf("%" SCNu64, &base[i]) != 1) return 2;
        for (unsigned i = 0; i < count; ++i)
            if (scanf("%" SCNu64, &stride[i]) != 1) return 2;
        for (unsigned i = 0; i < count; ++i)
            if (scanf("%" SCNu32, &align[i]) != 1) return 2;
        cap::QueryRange r[4];
        for (unsigned i = 0; i < count; ++i) r[i] = cap::QueryRange{names[i], (uintptr_t)base[i], stride[i], align[i], stride[i] != 0};
        char msg[256];
        if (cap::query_ranges_ok("cap_debug_query_ranges", n, r, count, msg, sizeof(msg)))
            puts("0");
        else
            printf("1 %s\n", msg);
    }
    return 0;
}
