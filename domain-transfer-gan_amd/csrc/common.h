// Shared helpers for libacgan_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include "../../include/acgan_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

void acg_set_error(const char *fmt, ...);
void acg_note_kernel(const char *fmt, ...);
extern int g_acg_conv_impl;
void acg_record_mid_event(hipStream_t st);   // acg_debug_mid_event: bench.py times a main kernel and its reduction apart

#define ACG_REQUIRE(cond, ...)                 \
    do {                                       \
        if (!(cond)) {                         \
            acg_set_error(__VA_ARGS__);        \
            return ACG_ERR_INVALID;            \
        }                                      \
    } while (0)

#define ACG_CHECK_LAUNCH(name)                                                     \
    do {                                                                           \
        hipError_t e__ = hipGetLastError();                                        \
        if (e__ != hipSuccess) {                                                   \
            acg_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));  \
            return ACG_ERR_LAUNCH;                                                 \
        }                                                                          \
    } while (0)

static inline int acg_cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline size_t acg_round_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

__device__ __forceinline__ float acg_apply_act(float v, int act)
{
    switch (act) {
    case ACG_ACT_RELU: return v > 0.f ? v : 0.f;
    case ACG_ACT_LRELU: return v > 0.f ? v : 0.2f * v;
    case ACG_ACT_TANH: return tanhf(v);
    default: return v;
    }
}
// d(act)/d(pre) expressed through the OUTPUT y (what the backward pass has at hand)
__device__ __forceinline__ float acg_act_grad_from_y(float y, int act)
{
    switch (act) {
    case ACG_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case ACG_ACT_LRELU: return y > 0.f ? 1.f : 0.2f;
    case ACG_ACT_TANH: return 1.f - y * y;
    default: return 1.f;
    }
}
// The convolution epilogues' activation argument: the acg_act kind in the low byte; a sigmoid carries the real output channel
// count above it (acg_act_sigmoid_ch).  Every other activation maps the zero of a padded channel to zero, the sigmoid would
// store 0.5 there — the epilogue writes exactly 0 instead (padded channels hold zeros).  Packed into `act` rather than a
// field of its own: a larger Geom moves the kernel arguments of every convolution kernel.
__host__ __device__ __forceinline__ int acg_act_kind(int act) { return act & 0xff; }
static inline int acg_act_sigmoid_ch(int creal) { return ACG_ACT_SIGMOID | (creal << 8); }
// The sigmoid is kept out of acg_apply_act / acg_act_grad_from_y: their run-time switch is inlined into every convolution
// epilogue, and a case more there changed the register allocation of kernels that never see a sigmoid.  The paths a sigmoid
// can reach (the head epilogues below, the dense layers, activation backward) call the _s variants.
__device__ __forceinline__ float acg_apply_act_s(float v, int act)
{
    return act == ACG_ACT_SIGMOID ? 1.f / (1.f + expf(-v)) : acg_apply_act(v, act);
}
__device__ __forceinline__ float acg_act_grad_from_y_s(float y, int act)
{
    return act == ACG_ACT_SIGMOID ? y * (1.f - y) : acg_act_grad_from_y(y, act);
}
__device__ __forceinline__ float acg_apply_act_ch(float v, int act, int c)
{
    if (acg_act_kind(act) == ACG_ACT_SIGMOID) return c >= (act >> 8) ? 0.f : acg_apply_act_s(v, ACG_ACT_SIGMOID);
    return acg_apply_act(v, act);
}
