// Shared by the two MFMA GEMM kernels (gemm_bf16.hip, gemm_v2.hip): fragment
// types, the bias/activation/store epilogue and the runtime → template
// dispatch of its three switches.
#pragma once

#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Store one 16x16 accumulator fragment of v_mfma_f32_16x16x32_bf16.
// C/D layout (guide §3): this lane holds column `col` (fragment col lane&15)
// of rows row0 + 0..3, where row0 = fragment row (lane>>4)*4.
template <int ACT, bool OUT_BF16, bool HAS_BIAS>
__device__ __forceinline__ void store_frag(f32x4 acc, const float* bias,
                                           void* C, int N, int row0, int col) {
    float b = HAS_BIAS ? bias[col] : 0.0f;
    #pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        int row = row0 + reg;
        float v = apply_act<ACT>(acc[reg] + b);
        if constexpr (OUT_BF16)
            ((short*)C)[(size_t)row * N + col] = f_to_bf16(v);
        else
            ((float*)C)[(size_t)row * N + col] = v;
    }
}

// Compile-time epilogue choice handed to a launcher by dispatch_epilogue.
template <int ACT, bool OUT_BF16, bool HAS_BIAS>
struct Epilogue {
    static constexpr int act = ACT;
    static constexpr bool out_bf16 = OUT_BF16;
    static constexpr bool has_bias = HAS_BIAS;
};

template <int ACT, typename Launch>
static inline void dispatch_out_bias(bool out_bf16, bool has_bias, Launch&& launch) {
    if (out_bf16) {
        if (has_bias) launch(Epilogue<ACT, true, true>{}); else launch(Epilogue<ACT, true, false>{});
    } else {
        if (has_bias) launch(Epilogue<ACT, false, true>{}); else launch(Epilogue<ACT, false, false>{});
    }
}

// Calls launch(Epilogue<...>{}) for the runtime (act, out_bf16, has_bias);
// returns FORGE_ERR_ACT for an unknown activation, else the launch status.
template <typename Launch>
static inline int dispatch_epilogue(int act, bool out_bf16, bool has_bias, Launch&& launch) {
    switch (act) {
        case FORGE_ACT_NONE: dispatch_out_bias<FORGE_ACT_NONE>(out_bf16, has_bias, launch); break;
        case FORGE_ACT_GELU: dispatch_out_bias<FORGE_ACT_GELU>(out_bf16, has_bias, launch); break;
        case FORGE_ACT_SIGMOID: dispatch_out_bias<FORGE_ACT_SIGMOID>(out_bf16, has_bias, launch); break;
        default: return FORGE_ERR_ACT;
    }
    return (int)hipGetLastError();
}
