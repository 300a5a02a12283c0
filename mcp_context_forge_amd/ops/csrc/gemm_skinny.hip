// bf16 MFMA GEMM for skinny M (C = A @ B^T, M <= ~1k): 64×64 tiles so that the
// classifier shapes fill the chip.
//
// gemm_v2's 256² tile gives (M=1024, N=1024) 16 workgroups on 256 CUs and
// gemm_bf16's 128² tile gives the 128-row rescan 8; either way one
// workgroup's serial K loop is the kernel's whole duration. Here the tile is
// 64×64: 256 workgroups at (1024, 1024), 32 at (128, 1024), no K split.
//
// Geometry: BM=BN=64, BK=64 (128-byte rows, so both operands are staged in
// full 128-byte lines), 256 threads = 4 waves (2×2), 32×32 = 2×2 fragments of
// 16×16 per wave. LDS = 4-slot ring × (A 8 KB + B 8 KB) = 64 KB in ONE
// __shared__ array: two workgroups fit a CU.
//
// Schedule: tiles 0..2 are staged in the prologue; iteration kt issues the
// four global_load_lds of tile kt+3 (into the slot tile kt-1 was read from,
// freed by the barrier that ended iteration kt-1), then runs tile kt's two
// K-steps. The only synchronisation is at the tile boundary: a counted
// `s_waitcnt vmcnt(N)` retires tile kt+1 while the later tiles stay in
// flight (N = 4 loads × tiles still ahead: 8, 4, then 0 at the drain), then
// one raw barrier.
//
// LDS swizzle as in gemm_bf16.hip: physical = logical ^ ((row & 7) << 4) on
// the 128-byte rows, applied to the global SOURCE address when staging (the
// LDS destination of global_load_lds is lane-linear) and to the LDS address
// when reading fragments.
//
// Numerics: every 16×16 fragment is ONE accumulator chain of
// v_mfma_f32_16x16x32_bf16 over K ascending in steps of 32, then store_frag:
// exactly what gemm_bf16.hip and gemm_v2.hip do, so results are bit-identical
// to both.
//
// Preconditions: M%64==0, N%64==0, K%64==0.

#include "gemm_common.h"

#define SK_BM 64
#define SK_BN 64
#define SK_BK 64                         // bf16 elems; 128 bytes per row
#define SK_ROWB (SK_BK * 2)
#define SK_SLOT_A (SK_BM * SK_ROWB)      // 8 KB
#define SK_SLOT_B (SK_BN * SK_ROWB)      // 8 KB
#define SK_RING 4                        // LDS slots (power of two)
#define SK_AHEAD 3                       // tiles staged ahead of the one computed

__device__ __forceinline__ uint32_t swz_sk(uint32_t byte_off) {
    return byte_off ^ (((byte_off >> 7) & 7u) << 4);
}

template <int ACT, bool OUT_BF16, bool HAS_BIAS>
__global__ __launch_bounds__(256, 2) void gemm_bt_skinny_kernel(
    const short* __restrict__ A,   // [M,K] bf16
    const short* __restrict__ BT,  // [N,K] bf16
    const float* __restrict__ bias,
    void* __restrict__ C,
    int M, int N, int K)
{
    // LDS ring: A slots [4][8KB] then B slots [4][8KB]
    __shared__ short lds[SK_RING * (SK_SLOT_A + SK_SLOT_B) / 2];
    char* lds_a = (char*)lds;
    char* lds_b = (char*)lds + SK_RING * SK_SLOT_A;

    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = tid >> 6;       // 0..3
    const int wm = wave >> 1;        // 0..1
    const int wn = wave & 1;         // 0..1
    const int tile_m = blockIdx.x * SK_BM;
    const int tile_n = blockIdx.y * SK_BN;
    const int n_tiles = K / SK_BK;

    f32x4 acc[2][2];
    #pragma unroll
    for (int i = 0; i < 2; ++i)
        #pragma unroll
        for (int j = 0; j < 2; ++j)
            acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- staging: 2 A-loads + 2 B-loads of 16 B per thread per tile ----
    // load i writes the linear LDS byte P = (i*256 + tid)*16 of the slot; the
    // data fetched is the logical offset swz_sk(P).
    auto stage_tile = [&](int t) {
        const int slot = t & (SK_RING - 1);
        #pragma unroll
        for (int i = 0; i < 2; ++i) {
            uint32_t P = (uint32_t)(i * 256 + tid) * 16u;
            uint32_t L = swz_sk(P);
            uint32_t row = L >> 7, colb = L & 127u;
            const short* gA = A + ((size_t)(tile_m + row) * K + t * SK_BK) + (colb >> 1);
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) uint32_t*)gA,
                (__attribute__((address_space(3))) uint32_t*)(lds_a + (size_t)slot * SK_SLOT_A
                                                              + (i * 256 + (wave * 64)) * 16),
                16, 0, 0);
        }
        #pragma unroll
        for (int i = 0; i < 2; ++i) {
            uint32_t P = (uint32_t)(i * 256 + tid) * 16u;
            uint32_t L = swz_sk(P);
            uint32_t row = L >> 7, colb = L & 127u;
            const short* gB = BT + ((size_t)(tile_n + row) * K + t * SK_BK) + (colb >> 1);
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) uint32_t*)gB,
                (__attribute__((address_space(3))) uint32_t*)(lds_b + (size_t)slot * SK_SLOT_B
                                                              + (i * 256 + (wave * 64)) * 16),
                16, 0, 0);
        }
    };
    // retire every tile but the `ahead` newest (4 loads per tile per thread)
    auto wait_tiles = [&](int ahead) {
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };

    // ---- prologue: stage tiles 0..AHEAD-1, retire tile 0 ----
    #pragma unroll
    for (int t = 0; t < SK_AHEAD; ++t)
        if (t < n_tiles) stage_tile(t);
    wait_tiles(min(SK_AHEAD, n_tiles) - 1);
    __builtin_amdgcn_s_barrier();

    const uint32_t k_col = (uint32_t)((lane >> 4) * 16);  // byte col of this lane's k-slice
    const uint32_t a_row_base = (uint32_t)(wm * 32 + (lane & 15));
    const uint32_t b_row_base = (uint32_t)(wn * 32 + (lane & 15));

    for (int kt = 0; kt < n_tiles; ++kt) {
        const char* slot_a = lds_a + (size_t)(kt & (SK_RING - 1)) * SK_SLOT_A;
        const char* slot_b = lds_b + (size_t)(kt & (SK_RING - 1)) * SK_SLOT_B;

        if (kt + SK_AHEAD < n_tiles) stage_tile(kt + SK_AHEAD);

        #pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 a_frag[2], b_frag[2];
            #pragma unroll
            for (int f = 0; f < 2; ++f) {
                uint32_t ra = a_row_base + f * 16, rb = b_row_base + f * 16;
                a_frag[f] = *(const bf16x8*)(slot_a + swz_sk(ra * SK_ROWB + kk * 64 + k_col));
                b_frag[f] = *(const bf16x8*)(slot_b + swz_sk(rb * SK_ROWB + kk * 64 + k_col));
            }
            #pragma unroll
            for (int fr = 0; fr < 2; ++fr)
                #pragma unroll
                for (int fc = 0; fc < 2; ++fc)
                    acc[fr][fc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag[fr], b_frag[fc], acc[fr][fc], 0, 0, 0);
        }
        // tile boundary: retire tile kt+1; the tiles after it stay in flight
        if (kt + 1 < n_tiles) {
            wait_tiles(min(kt + SK_AHEAD, n_tiles - 1) - (kt + 1));
            __builtin_amdgcn_s_barrier();
        }
    }

    // ---- epilogue ----
    #pragma unroll
    for (int fr = 0; fr < 2; ++fr) {
        #pragma unroll
        for (int fc = 0; fc < 2; ++fc) {
            int col = tile_n + wn * 32 + fc * 16 + (lane & 15);
            int row0 = tile_m + wm * 32 + fr * 16 + (lane >> 4) * 4;
            store_frag<ACT, OUT_BF16, HAS_BIAS>(acc[fr][fc], bias, C, N, row0, col);
        }
    }
}

extern "C" int forge_gemm_bt_skinny(
    const void* A, const void* BT, const void* bias, void* C,
    int M, int N, int K, int act, int out_bf16, void* stream)
{
    if (M <= 0 || N <= 0 || K <= 0 || (M % SK_BM) || (N % SK_BN) || (K % SK_BK)) return FORGE_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(M / SK_BM, N / SK_BN);
    return dispatch_epilogue(act, out_bf16 != 0, bias != nullptr, [&](auto e) {
        using E = decltype(e);
        hipLaunchKernelGGL((gemm_bt_skinny_kernel<E::act, E::out_bf16, E::has_bias>), grid, dim3(256), 0, s,
                           (const short*)A, (const short*)BT, (const float*)bias, C, M, N, K);
    });
}
