// The naive "direct" kernels (ACG_IMPL_DIRECT), kept as an on-device cross-check of the MFMA path: one thread per output
// element, geometry taken straight from the descriptor (independent of the tap-list machinery).
#include "conv_internal.h"

__device__ __forceinline__ int reflect_idx(int i, int n) { i = i < 0 ? -i : i; return i >= n ? 2 * (n - 1) - i : i; }

__global__ void direct_fwd_kernel(acg_conv_desc d, const float *__restrict__ x, const float *__restrict__ wf,
                                  const float *__restrict__ bias, float *__restrict__ y, int act, int CoP)
{
    const long long total = (long long)d.N * d.Ho * d.Wo * d.Co;
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    long long r = i;
    const int co = (int)(r % d.Co); r /= d.Co;
    const int ox = (int)(r % d.Wo); r /= d.Wo;
    const int oy = (int)(r % d.Ho); r /= d.Ho;
    const int n = (int)r;
    float acc = bias ? bias[co] : 0.f;
    for (int kh = 0; kh < d.K; ++kh)
        for (int kw = 0; kw < d.K; ++kw) {
            int iy = oy * d.stride + kh - d.pad, ix = ox * d.stride + kw - d.pad;
            if (d.pad_mode == ACG_PAD_REFLECT) {
                iy = reflect_idx(iy, d.Hi);
                ix = reflect_idx(ix, d.Wi);
            } else if (iy < 0 || iy >= d.Hi || ix < 0 || ix >= d.Wi)
                continue;
            const float *xp = x + (((long long)n * d.Hi + iy) * d.Wi + ix) * d.Ci;
            const int tap = kh * d.K + kw;
            for (int ci = 0; ci < d.Ci; ++ci)
                acc += xp[ci] * wf[(((long long)tap * (c16(d.Ci) / 8) + ci / 8) * CoP + co) * 8 + (ci & 7)];
        }
    y[i] = act == ACG_ACT_SIGMOID && co >= (d.Cor > 0 ? d.Cor : d.Co) ? 0.f : acg_apply_act_s(acc, act);
}

// dx[n,iy,ix,ci] = sum over padded preimages (py,px), taps, co.  Also used (with bias/act) as the
// ConvTranspose2d forward.
__global__ void direct_dgrad_kernel(acg_conv_desc d, const float *__restrict__ dy, const float *__restrict__ wb,
                                    const float *__restrict__ bias, float *__restrict__ dx, int act, int CiP)
{
    const long long total = (long long)d.N * d.Hi * d.Wi * d.Ci;
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    long long r = i;
    const int ci = (int)(r % d.Ci); r /= d.Ci;
    const int ix = (int)(r % d.Wi); r /= d.Wi;
    const int iy = (int)(r % d.Hi); r /= d.Hi;
    const int n = (int)r;
    const int p = d.pad;
    int ys[3], xs[3], ny = 0, nx = 0;
    ys[ny++] = iy + p;
    xs[nx++] = ix + p;
    if (d.pad_mode == ACG_PAD_REFLECT) {
        if (iy >= 1 && iy <= p) ys[ny++] = p - iy;
        if (iy >= d.Hi - 1 - p && iy <= d.Hi - 2) ys[ny++] = 2 * (d.Hi - 1) - iy + p;
        if (ix >= 1 && ix <= p) xs[nx++] = p - ix;
        if (ix >= d.Wi - 1 - p && ix <= d.Wi - 2) xs[nx++] = 2 * (d.Wi - 1) - ix + p;
    }
    float acc = bias ? bias[ci] : 0.f;
    for (int a = 0; a < ny; ++a)
        for (int b = 0; b < nx; ++b)
            for (int kh = 0; kh < d.K; ++kh)
                for (int kw = 0; kw < d.K; ++kw) {
                    const int ty = ys[a] - kh, tx = xs[b] - kw;
                    if (ty < 0 || tx < 0 || ty % d.stride || tx % d.stride) continue;
                    const int oy = ty / d.stride, ox = tx / d.stride;
                    if (oy >= d.Ho || ox >= d.Wo) continue;
                    const float *gp = dy + (((long long)n * d.Ho + oy) * d.Wo + ox) * d.Co;
                    const int tap = kh * d.K + kw;
                    for (int co = 0; co < d.Co; ++co)
                        acc += gp[co] * wb[(((long long)tap * (c16(d.Co) / 8) + co / 8) * CiP + ci) * 8 + (co & 7)];
                }
    dx[i] = acg_apply_act(acc, act);
}

// dw[o][i][kh][kw] (real Or x Ir), one thread per weight, serial over all pixels (tests only)
__global__ void direct_wgrad_kernel(acg_conv_desc d, const float *__restrict__ x, const float *__restrict__ dy,
                                    float *__restrict__ dw, int Or, int Ir, int accumulate)
{
    const int KK = d.K * d.K;
    const long long total = (long long)Or * Ir * KK;
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    long long r = i;
    const int tap = (int)(r % KK); r /= KK;
    const int ci = (int)(r % Ir); r /= Ir;
    const int co = (int)r;
    const int kh = tap / d.K, kw = tap % d.K;
    float acc = 0.f;
    for (int n = 0; n < d.N; ++n)
        for (int oy = 0; oy < d.Ho; ++oy)
            for (int ox = 0; ox < d.Wo; ++ox) {
                int iy = oy * d.stride + kh - d.pad, ix = ox * d.stride + kw - d.pad;
                if (d.pad_mode == ACG_PAD_REFLECT) {
                    iy = reflect_idx(iy, d.Hi);
                    ix = reflect_idx(ix, d.Wi);
                } else if (iy < 0 || iy >= d.Hi || ix < 0 || ix >= d.Wi)
                    continue;
                acc += x[(((long long)n * d.Hi + iy) * d.Wi + ix) * d.Ci + ci] *
                       dy[(((long long)n * d.Ho + oy) * d.Wo + ox) * d.Co + co];
            }
    dw[i] = (accumulate ? dw[i] : 0.f) + acc;
}

int acg_direct_fwd_launch(const acg_conv_desc *d, const float *x, const float *wf, const float *bias, float *y, int act, hipStream_t st)
{
    const long long total = (long long)d->N * d->Ho * d->Wo * d->Co;
    hipLaunchKernelGGL(direct_fwd_kernel, dim3(acg_cdiv(total, 256)), dim3(256), 0, st, *d, x, wf, bias, y, act, acg_ncols_pad(d->Co));
    ACG_CHECK_LAUNCH("direct_fwd_kernel");
    acg_note_kernel("direct_fwd_kernel");
    return ACG_OK;
}
int acg_direct_dgrad_launch(const acg_conv_desc *d, const float *dy, const float *wb, const float *bias, float *dx, int act, hipStream_t st)
{
    const long long total = (long long)d->N * d->Hi * d->Wi * d->Ci;
    hipLaunchKernelGGL(direct_dgrad_kernel, dim3(acg_cdiv(total, 256)), dim3(256), 0, st, *d, dy, wb, bias, dx, act, acg_ncols_pad(d->Ci));
    ACG_CHECK_LAUNCH("direct_dgrad_kernel");
    return ACG_OK;
}
int acg_direct_wgrad_launch(const acg_conv_desc *d, const float *x, const float *dy, float *dw, int Or, int Ir, int accumulate, hipStream_t st)
{
    const long long total = (long long)Or * Ir * d->K * d->K;
    hipLaunchKernelGGL(direct_wgrad_kernel, dim3(acg_cdiv(total, 64)), dim3(64), 0, st, *d, x, dy, dw, Or, Ir, accumulate);
    ACG_CHECK_LAUNCH("direct_wgrad_kernel");
    return ACG_OK;
}
