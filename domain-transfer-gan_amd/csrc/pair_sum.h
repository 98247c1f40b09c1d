// The deterministic sum of a pair of doubles over a workgroup and over a row of partial pairs: what makes ssim.hip, crps.hip,
// fss_loss.hip and marginal.hip give the same bits on every call and in every layout of their operands.  Every sum has a fixed
// shape: a shuffle tree per wave (offsets 32 .. 1), then the waves in order from 0.0 by thread 0.  Additions only: an
// including file's `fp contract` state has nothing to act on here.
#pragma once
#include <hip/hip_runtime.h>

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// the sums of a and of b over the THREADS threads of the workgroup -> finish(sum a, sum b) on thread 0.  Every thread of the
// workgroup must call it.  red may be reused call after call: the first barrier lets the previous call's reader (and whoever
// else read LDS before the call) finish first.
template <int THREADS, typename Finish>
__device__ __forceinline__ void pair_block_sum(double a, double b, double (*red)[THREADS / 64], Finish finish)
{
    a = wave_sum(a), b = wave_sum(b);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[0][wave] = a, red[1][wave] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0.0, s1 = 0.0;
        for (int w = 0; w < THREADS / 64; ++w) s0 += red[0][w], s1 += red[1][w];
        finish(s0, s1);
    }
}

// ... stored as they are: out[0], out[1]
template <int THREADS>
__device__ __forceinline__ void pair_block_store(double a, double b, double (*red)[THREADS / 64], double *out)
{
    pair_block_sum<THREADS>(a, b, red, [=](double s0, double s1) { out[0] = s0, out[1] = s1; });
}

// the fold of a launch of one wave per group: group blockIdx.x owns the n partial pairs at part + blockIdx.x * n * 2.  Lane l
// sums pairs l, l + 64, .. in that order, then the shuffle tree -> finish(sum of the firsts, sum of the seconds) on lane 0.
template <typename Finish>
__device__ __forceinline__ void pair_fold(const double *__restrict__ part, int n, Finish finish)
{
    const double *p = part + (long long)blockIdx.x * n * 2;
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) s0 += p[2 * i], s1 += p[2 * i + 1];
    s0 = wave_sum(s0), s1 = wave_sum(s1);
    if (threadIdx.x == 0) finish(s0, s1);
}
