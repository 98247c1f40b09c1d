// What spectrum.hip and field_spectrum.hip share beyond field.h: the integer root of the ring rules and the twiddle tables
// of the radix-2 Stockham stages.  Their butterflies, products and ring enumerators are their own: the two files pin
// different fused multiply-add choices, and their bits are asserted.
#pragma once
#include <math.h>
#include "common.h"

__host__ __device__ __forceinline__ int spec_isqrt(int n)         // floor(sqrt(n)), 0 <= n < 2^24
{
    int r = (int)sqrtf((float)n);
    while (r * r > n) --r;
    while ((r + 1) * (r + 1) <= n) ++r;
    return r;
}

// tw[Ns + k] = exp(-i pi k / Ns), 0 <= k < Ns, Ns = 1, 2, .. M/2: stage Ns reads tw[Ns + (j mod Ns)]; exact arguments
__device__ __forceinline__ void spec_twiddles(float2 *tw, int M)
{
    for (int m = threadIdx.x + 1; m < M; m += blockDim.x) {
        const int Ns = 1 << (31 - __clz(m)), k = m - Ns;
        float s, c;
        sincospif(-(float)k / (float)Ns, &s, &c);
        tw[m] = make_float2(c, s);
    }
}
