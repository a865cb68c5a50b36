// cap_wide_quant.h — the quantiser of the compressed 8-wide view (cap_wide.h): grid origin, steps and child planes of one node
// from its padded child boxes in double precision.  Shared by the device collapse (bvh.hip k_wide_level) and the refit
// (refit.hip k_wide_refit), so that a refit with unchanged positions reproduces the collapse byte for byte.  The host collapse
// (wide_builder.cpp Collapser::emit) does the same arithmetic.
#pragma once

#include "cap_device.h"
#include "cap_wide.h"

namespace cap
{
struct WideGrid
{
    float  p[3];     // grid origin
    double step[3];  // grid steps (powers of two)
};

// grid origin (the node's low corner rounded down to float) and steps (the smallest power of two with <= 255 steps): words 0..3, 7
__device__ __forceinline__ WideGrid wide_grid(const double nlo[3], const double nhi[3], uint32_t word[kWideNodeWords])
{
    WideGrid g;
    uint32_t eb[3];
    for (int k = 0; k < 3; ++k)
    {
        g.p[k] = (float)nlo[k];
        if ((double)g.p[k] > nlo[k]) g.p[k] = u2f(g.p[k] > 0.0f ? f2u(g.p[k]) - 1u : (g.p[k] < 0.0f ? f2u(g.p[k]) + 1u : 0x80000001u));  // next float down
        word[k] = f2u(g.p[k]);
        const double ext = nhi[k] - (double)g.p[k];
        int          e   = -100;
        if (ext > 0.0)
        {
            int fe;
            (void)frexp(ext / 255.0, &fe);
            e = fe - 1 > -100 ? fe - 1 : -100;
        }
        while (ceil(ext / ldexp(1.0, e)) > 255.0) ++e;
        g.step[k] = ldexp(1.0, e);
        eb[k]     = (uint32_t)(e + 127);
    }
    word[3] = eb[0] << 23;
    word[7] = ((eb[1] << 23) & 0xffff0000u) | ((eb[2] << 23) >> 16);
    return g;
}

// slot s's planes (low rounded down, high rounded up, clamped to the grid) OR-ed into words 8..19
__device__ __forceinline__ void wide_quantise(const WideGrid& g, const double clo[3], const double chi[3], int s, uint32_t word[kWideNodeWords])
{
    for (int k = 0; k < 3; ++k)
    {
        double qlo = floor((clo[k] - (double)g.p[k]) / g.step[k]), qhi = ceil((chi[k] - (double)g.p[k]) / g.step[k]);
        qlo = fmin(fmax(qlo, 0.0), 255.0), qhi = fmin(fmax(qhi, 0.0), 255.0);
        const uint32_t wi = 8u + 2u * (uint32_t)k + ((uint32_t)s >> 2), sh = 8u * ((uint32_t)s & 3u);
        word[wi] |= (uint32_t)qlo << sh;
        word[wi + 6] |= (uint32_t)qhi << sh;
    }
}
}  // namespace cap
