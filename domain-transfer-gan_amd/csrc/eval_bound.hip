// The variational bound of the offline evaluator (evaluate.py:56-141, test.py:111-175): the per-sample pixel likelihood of
// an image under a Laplace or Gaussian model with a per-pixel log-variance plane, its gradients, and one launch for the latent
// tail of an iterate (KLD, trace row, gradient through the clamp of gauss_reparametrize, RMSprop, next z).
// Image tensors are NHWC with Cp stored channels (Cp a multiple of 4), C of them valid; logvar is ONE (npix, Cp) plane that is
// broadcast over the batch.  Every reduction runs in a fixed order: no float atomics, results are bit-identical on a repeat.
#include <math.h>
#include "common.h"

#define NLL_THREADS 256
#define NLL_PIX_PER_THREAD 4
#define NLL_CHUNK (NLL_THREADS * NLL_PIX_PER_THREAD) // pixels of one sample per partial-sum block

static constexpr float kLog2 = 0.69314718055994531f;          // log 2               (model.py:28)
static constexpr float kHalfLog2Pi = 0.91893853320467274f;    // 0.5 log(2 pi)       (model.py:34)

static inline long long nll_chunks(size_t npix) { return ((long long)npix + NLL_CHUNK - 1) / NLL_CHUNK; }

// -log p of one element: Laplace 0.5 lv + |x - mu| / exp(0.5 lv) + log 2, Gaussian 0.5 lv + (x - mu)^2 / (2 exp(lv)) + 0.5 log 2 pi
template <int KIND>
__device__ __forceinline__ float nll_term(float x, float m, float lv)
{
    const float d = x - m;
    if (KIND == ACG_NLL_LAPLACE) return (0.5f * lv + fabsf(d) / expf(0.5f * lv)) + kLog2;
    return (0.5f * lv + d * d / (2.f * expf(lv))) + kHalfLog2Pi;
}

// part[n * nchunk + blockIdx.x] = sum of nll_term over the valid channels of pixels [chunk * NLL_CHUNK, +NLL_CHUNK) of sample n
template <int KIND>
__global__ __launch_bounds__(NLL_THREADS) void pixel_nll_partial_kernel(const float *__restrict__ x, const float *__restrict__ mu,
                                                                        const float *__restrict__ logvar, long long npix, int C,
                                                                        int Cp, int nchunk, float *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ float red[NLL_THREADS];
    const int n = blockIdx.y, nq = Cp >> 2;
    const long long base = (long long)n * npix * Cp;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NLL_PIX_PER_THREAD; ++k) {
        const long long p = (long long)blockIdx.x * NLL_CHUNK + k * NLL_THREADS + threadIdx.x;
        if (p >= npix) break;
        for (int q = 0; q < nq; ++q) {
            const long long o = p * Cp + q * 4;
            const f32x4 xv = *(const f32x4 *)(x + base + o);
            const f32x4 mv = *(const f32x4 *)(mu + base + o);
            const f32x4 lv = *(const f32x4 *)(logvar + o);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (q * 4 + j < C) s += nll_term<KIND>(xv[j], mv[j], lv[j]);
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = NLL_THREADS / 2; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long long)n * nchunk + blockIdx.x] = red[0];
}

// out[n] = the chunk partials of sample n, folded in chunk order by one thread
__global__ __launch_bounds__(256) void pixel_nll_fold_kernel(const float *__restrict__ part, int N, int nchunk,
                                                             float *__restrict__ out)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int k = 0; k < nchunk; ++k) s += part[(long long)n * nchunk + k];
    out[n] = s;
}

extern "C" size_t acg_pixel_nll_workspace_bytes(int N, size_t npix)
{
    return (size_t)(N > 0 ? N : 0) * (size_t)nll_chunks(npix) * sizeof(float);
}

static int nll_args_ok(const char *who, int kind, const float *x, const float *mu, const float *logvar, int N, size_t npix, int C,
                       int Cp)
{
    ACG_REQUIRE(kind == ACG_NLL_LAPLACE || kind == ACG_NLL_GAUSSIAN, "%s: unknown kind %d", who, kind);
    ACG_REQUIRE(x && mu && logvar, "%s: null input", who);
    ACG_REQUIRE(N >= 1 && npix >= 1, "%s: empty tensor (N=%d, npix=%zu)", who, N, npix);
    ACG_REQUIRE(Cp >= 4 && Cp % 4 == 0 && C >= 1 && C <= Cp, "%s: need 1 <= C <= Cp, Cp a multiple of 4 (C=%d, Cp=%d)", who, C, Cp);
    ACG_REQUIRE(((uintptr_t)x | (uintptr_t)mu | (uintptr_t)logvar) % 16 == 0, "%s: tensors must be 16-byte aligned", who);
    return ACG_OK;
}

extern "C" int acg_pixel_nll_fwd(int kind, const float *x, const float *mu, const float *logvar, int N, size_t npix, int C, int Cp,
                                 float *out, void *ws, size_t ws_bytes, void *stream)
{
    const int rc = nll_args_ok("acg_pixel_nll_fwd", kind, x, mu, logvar, N, npix, C, Cp);
    if (rc != ACG_OK) return rc;
    ACG_REQUIRE(out != nullptr, "acg_pixel_nll_fwd: null output");
    const long long nchunk = nll_chunks(npix);
    ACG_REQUIRE(nchunk <= 65535 && N <= 65535, "acg_pixel_nll_fwd: too large (N=%d, npix=%zu)", N, npix);
    if (ws == nullptr || ws_bytes < acg_pixel_nll_workspace_bytes(N, npix)) {
        acg_set_error("acg_pixel_nll_fwd: workspace too small (%zu < %zu)", ws_bytes, acg_pixel_nll_workspace_bytes(N, npix));
        return ACG_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    float *part = (float *)ws;
    const dim3 grid((unsigned)nchunk, (unsigned)N);
    if (kind == ACG_NLL_LAPLACE)
        hipLaunchKernelGGL(pixel_nll_partial_kernel<ACG_NLL_LAPLACE>, grid, dim3(NLL_THREADS), 0, st, x, mu, logvar,
                           (long long)npix, C, Cp, (int)nchunk, part);
    else
        hipLaunchKernelGGL(pixel_nll_partial_kernel<ACG_NLL_GAUSSIAN>, grid, dim3(NLL_THREADS), 0, st, x, mu, logvar,
                           (long long)npix, C, Cp, (int)nchunk, part);
    hipLaunchKernelGGL(pixel_nll_fold_kernel, dim3(acg_cdiv(N, 256)), dim3(256), 0, st, (const float *)part, N, (int)nchunk, out);
    ACG_CHECK_LAUNCH("acg_pixel_nll_fwd");
    return ACG_OK;
}

// Per-element gradients of g * (-log p): inv_scale = 1 / exp(0.5 lv) (Laplace) or 1 / exp(lv) (Gaussian).
template <int KIND>
__device__ __forceinline__ float nll_inv_scale(float lv) { return KIND == ACG_NLL_LAPLACE ? 1.f / expf(0.5f * lv) : 1.f / expf(lv); }
template <int KIND>
__device__ __forceinline__ float nll_dmu(float d, float inv_scale, float g)
{
#pragma clang fp contract(off)
    // Laplace: d/dmu |x - mu| / sd = -sign(x - mu) / sd, sign(0) = 0 (torch's abs backward)
    if (KIND == ACG_NLL_LAPLACE) return d > 0.f ? -g * inv_scale : (d < 0.f ? g * inv_scale : 0.f);
    return g * (-d * inv_scale);
}
template <int KIND>
__device__ __forceinline__ float nll_dlv(float d, float inv_scale, float g)
{
#pragma clang fp contract(off)
    if (KIND == ACG_NLL_LAPLACE) return g * (0.5f - 0.5f * (fabsf(d) * inv_scale));
    return g * (0.5f - 0.5f * (d * d * inv_scale));
}

// dmu: one thread per (sample, pixel, group of 4 channels) — a grid as wide as the tensor
template <int KIND>
__global__ __launch_bounds__(256) void pixel_nll_dmu_kernel(const float *__restrict__ x, const float *__restrict__ mu,
                                                            const float *__restrict__ logvar, long long nq_total, long long plane_q,
                                                            int C, int nq, const float *__restrict__ g, float *__restrict__ dmu)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nq_total) return;
    const long long n = t / plane_q, tq = t - n * plane_q;     // tq: (pixel, quad) inside the sample
    const int c0 = (int)(tq % nq) * 4;
    const float gn = g[n];
    const f32x4 lv = *(const f32x4 *)(logvar + tq * 4);
    const f32x4 xv = *(const f32x4 *)(x + t * 4);
    const f32x4 mv = *(const f32x4 *)(mu + t * 4);
    f32x4 dm;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        dm[j] = c0 + j < C ? nll_dmu<KIND>(xv[j] - mv[j], nll_inv_scale<KIND>(lv[j]), gn) : 0.f;
    *(f32x4 *)(dmu + t * 4) = dm;
}

// dlogvar: one thread per (pixel, group of 4 channels) walks the batch in order and sums — no atomics
template <int KIND>
__global__ __launch_bounds__(256) void pixel_nll_dlogvar_kernel(const float *__restrict__ x, const float *__restrict__ mu,
                                                                const float *__restrict__ logvar, int N, long long plane_q,
                                                                int C, int nq, const float *__restrict__ g,
                                                                float *__restrict__ dlogvar)
{
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= plane_q) return;
    const int c0 = (int)(t % nq) * 4;
    const f32x4 lv = *(const f32x4 *)(logvar + t * 4);
    f32x4 inv_scale, dlv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        inv_scale[j] = nll_inv_scale<KIND>(lv[j]);
        dlv[j] = 0.f;
    }
    for (int n = 0; n < N; ++n) {
        const float gn = g[n];
        const f32x4 xv = *(const f32x4 *)(x + (n * plane_q + t) * 4);
        const f32x4 mv = *(const f32x4 *)(mu + (n * plane_q + t) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < C) dlv[j] += nll_dlv<KIND>(xv[j] - mv[j], inv_scale[j], gn);
    }
    *(f32x4 *)(dlogvar + t * 4) = dlv;
}

template <int KIND>
static void pixel_nll_bwd_launch(const float *x, const float *mu, const float *logvar, int N, long long plane_q, int C, int nq,
                                 const float *g, float *dmu, float *dlogvar, hipStream_t st)
{
    if (dmu) {
        const long long total = (long long)N * plane_q;
        hipLaunchKernelGGL(pixel_nll_dmu_kernel<KIND>, dim3(acg_cdiv(total, 256)), dim3(256), 0, st, x, mu, logvar, total, plane_q,
                           C, nq, g, dmu);
    }
    if (dlogvar)
        hipLaunchKernelGGL(pixel_nll_dlogvar_kernel<KIND>, dim3(acg_cdiv(plane_q, 256)), dim3(256), 0, st, x, mu, logvar, N,
                           plane_q, C, nq, g, dlogvar);
}

extern "C" int acg_pixel_nll_bwd(int kind, const float *x, const float *mu, const float *logvar, int N, size_t npix, int C, int Cp,
                                 const float *g, float *dmu, float *dlogvar, void *stream)
{
    const int rc = nll_args_ok("acg_pixel_nll_bwd", kind, x, mu, logvar, N, npix, C, Cp);
    if (rc != ACG_OK) return rc;
    ACG_REQUIRE(g != nullptr, "acg_pixel_nll_bwd: null g");
    ACG_REQUIRE(((uintptr_t)dmu | (uintptr_t)dlogvar) % 16 == 0, "acg_pixel_nll_bwd: outputs must be 16-byte aligned");
    const long long plane_q = (long long)npix * (Cp / 4);
    ACG_REQUIRE((long long)N * plane_q / 256 < 0x7fffffffLL, "acg_pixel_nll_bwd: too large (N=%d, npix=%zu)", N, npix);
    hipStream_t st = (hipStream_t)stream;
    if (kind == ACG_NLL_LAPLACE)
        pixel_nll_bwd_launch<ACG_NLL_LAPLACE>(x, mu, logvar, N, plane_q, C, Cp / 4, g, dmu, dlogvar, st);
    else
        pixel_nll_bwd_launch<ACG_NLL_GAUSSIAN>(x, mu, logvar, N, plane_q, C, Cp / 4, g, dmu, dlogvar, st);
    ACG_CHECK_LAUNCH("acg_pixel_nll_bwd");
    return ACG_OK;
}

// ---------------------------------------------------------------- the latent tail of one bound iterate (one workgroup)
#define LBS_THREADS 256
__device__ __forceinline__ float reparam_pre(float e, float m, float lv)
{
#pragma clang fp contract(off)
    return e * expf(0.5f * lv) + m;       // eps * std + mu, rounded as torch's mul then add (model.py:15-22)
}
__device__ __forceinline__ float clamp4(float v) { return v < -4.f ? -4.f : (v > 4.f ? 4.f : v); }

__global__ __launch_bounds__(LBS_THREADS) void latent_bound_step_kernel(int N, int L, float ubo_const, double bpp_den,
                                                                        float *__restrict__ mu, float *__restrict__ logvar,
                                                                        float *__restrict__ sq_mu, float *__restrict__ sq_logvar,
                                                                        const float *__restrict__ eps, const float *__restrict__ dz,
                                                                        const float *__restrict__ nll, float lr, float alpha,
                                                                        float rms_eps, float *__restrict__ trace_row,
                                                                        const float *__restrict__ eps_next,
                                                                        float *__restrict__ z_next)
{
#pragma clang fp contract(off)
    __shared__ double red[2][LBS_THREADS];
    const int tid = threadIdx.x;
    const long long total = (long long)N * L;
    if (dz != nullptr) {
        // 1-2: KLD of the current (mu, logvar) per sample (model.py:45-53), the bound nll + kld + npx log 127.5
        // (evaluate.py:93-109); means over the batch into the trace row
        double s_ubo = 0.0, s_kld = 0.0;
        for (int n = tid; n < N; n += LBS_THREADS) {
            float k = 0.f;
            for (int l = 0; l < L; ++l) {
                const float m = mu[(long long)n * L + l], lv = logvar[(long long)n * L + l];
                k += ((lv + 1.f) - m * m) - expf(lv);
            }
            k *= -0.5f;
            s_kld += (double)k;
            s_ubo += (double)((nll[n] + k) + ubo_const);
        }
        red[0][tid] = s_ubo;
        red[1][tid] = s_kld;
        __syncthreads(); // also orders every read of (mu, logvar) above before the in-place update below
        for (int k = LBS_THREADS / 2; k > 0; k >>= 1) {
            if (tid < k) {
                red[0][tid] += red[0][tid + k];
                red[1][tid] += red[1][tid + k];
            }
            __syncthreads();
        }
        if (tid == 0 && trace_row != nullptr) {
            const float ubo = (float)(red[0][0] / N), kld = (float)(red[1][0] / N);
            trace_row[0] = ubo;
            trace_row[1] = kld;
            trace_row[2] = (float)((double)ubo / bpp_den);
        }
    }
    const float invN = 1.f / (float)N, b = 1.f - alpha;
    for (long long e = tid; e < total; e += LBS_THREADS) {
        float m = mu[e], lv = logvar[e];
        if (dz != nullptr) {
            // 3: d mean(ubo) / d(mu, logvar): through z = clamp(eps exp(0.5 lv) + mu, -4, 4) — the gradient passes where
            // -4 <= pre <= 4, inclusive (torch's clamp backward) — plus the KLD's own term / N
            const float ep = eps[e], sd = expf(0.5f * lv), pre = ep * sd + m;
            const float gz = (pre >= -4.f && pre <= 4.f) ? dz[e] : 0.f;
            const float gm = gz + m * invN;
            const float gl = ((gz * ep) * sd) * 0.5f + (0.5f * (expf(lv) - 1.f)) * invN;
            // 4: torch.optim.RMSprop (no momentum, not centred): sq = alpha sq + (1 - alpha) g^2, p -= lr g / (sqrt(sq) + eps)
            const float sm = alpha * sq_mu[e] + b * (gm * gm), sl = alpha * sq_logvar[e] + b * (gl * gl);
            sq_mu[e] = sm;
            sq_logvar[e] = sl;
            m = m - lr * (gm / (sqrtf(sm) + rms_eps));
            lv = lv - lr * (gl / (sqrtf(sl) + rms_eps));
            mu[e] = m;
            logvar[e] = lv;
        }
        // 5: the next iterate's code
        if (eps_next != nullptr) z_next[e] = clamp4(reparam_pre(eps_next[e], m, lv));
    }
}

extern "C" int acg_latent_bound_step(int N, int L, int npx, float *mu, float *logvar, float *sq_mu, float *sq_logvar,
                                     const float *eps, const float *dz, const float *nll, float lr, float alpha, float rms_eps,
                                     float *trace_row, const float *eps_next, float *z_next, void *stream)
{
    ACG_REQUIRE(N >= 1 && L >= 1 && npx >= 1, "acg_latent_bound_step: bad sizes N=%d L=%d npx=%d", N, L, npx);
    ACG_REQUIRE(mu && logvar, "acg_latent_bound_step: null mu / logvar");
    ACG_REQUIRE(dz == nullptr || (sq_mu && sq_logvar && eps && nll), "acg_latent_bound_step: an update needs sq_mu, sq_logvar, "
                "eps and nll");
    ACG_REQUIRE((eps_next == nullptr) == (z_next == nullptr), "acg_latent_bound_step: eps_next and z_next go together");
    const double c = (double)npx;
    hipLaunchKernelGGL(latent_bound_step_kernel, dim3(1), dim3(LBS_THREADS), 0, (hipStream_t)stream, N, L,
                       (float)(c * log(127.5)), c * log(2.0), mu, logvar, sq_mu, sq_logvar, eps, dz, nll, lr, alpha,
                       rms_eps, trace_row, eps_next, z_next);
    ACG_CHECK_LAUNCH("acg_latent_bound_step");
    return ACG_OK;
}
