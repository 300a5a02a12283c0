// Shared helpers for the MI355X (gfx950 / CDNA4) gateway kernels.
// Compile: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "forge_api.h"

#define WAVE 64  // CDNA wavefront width (hard-coded per guide: warpSize==64 on gfx950)

// 8 x bf16 stored as shorts — the vectorized load unit (guide G13).
typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(4))) float float4v;

__device__ __forceinline__ float bf16_to_f(short s) {
    union { float f; uint32_t u; } cvt;
    cvt.u = ((uint32_t)(uint16_t)s) << 16;
    return cvt.f;
}

__device__ __forceinline__ short f_to_bf16(float f) {
    union { float f; uint32_t u; } cvt;
    cvt.f = f;
    // round-to-nearest-even
    uint32_t lsb = (cvt.u >> 16) & 1;
    cvt.u += 0x7fff + lsb;
    return (short)(cvt.u >> 16);
}

__device__ __forceinline__ float gelu_tanh(float x) {
    // matches torch.nn.functional.gelu(approximate="tanh")
    const float c = 0.7978845608028654f;  // sqrt(2/pi)
    float x3 = x * x * x;
    return 0.5f * x * (1.0f + tanhf(c * (x + 0.044715f * x3)));
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int ACT>
__device__ __forceinline__ float apply_act(float v) {
    if constexpr (ACT == FORGE_ACT_GELU) v = gelu_tanh(v);
    if constexpr (ACT == FORGE_ACT_SIGMOID) v = sigmoidf(v);
    return v;
}

// Sum over the wave; the total is valid in lane 0 (shfl_down by 32..1).
__device__ __forceinline__ float wave_sum(float v) {
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// One wave's bf16 dot of two K-element rows (K % 8 == 0, 16-byte aligned):
// lane-strided 8-element chunks accumulated in element order, then wave_sum.
__device__ __forceinline__ float wave_dot_bf16(const short* __restrict__ a_row,
                                               const short* __restrict__ b_row, int K, int lane) {
    float dot = 0.0f;
    for (int k = lane * 8; k < K; k += WAVE * 8) {
        short8 av = *(const short8*)(a_row + k);
        short8 bv = *(const short8*)(b_row + k);
        #pragma unroll
        for (int j = 0; j < 8; ++j) dot += bf16_to_f(av[j]) * bf16_to_f(bv[j]);
    }
    return wave_sum(dot);
}

static inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
