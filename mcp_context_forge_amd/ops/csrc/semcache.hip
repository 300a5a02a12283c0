// Identity-aware top-k lookup of the HBM semantic cache: the sketch sweep fused
// with the eligibility filter and the selection (forge_sketch_topk), and the
// exact full-dimension check of the k candidates (forge_verify_topk).
//
// ---- sketch_topk_kernel ----
// A workgroup owns one 64-row query tile and a contiguous range of 64-slot
// tiles of the sketch matrix: grid (B/64, splits). 256 threads = 4 waves (2×2),
// each wave 2×2 fragments of v_mfma_f32_16x16x32_bf16, ONE accumulator chain
// per fragment over K ascending in steps of 32: the chain of gemm_skinny.hip,
// so every score has the bits hip.gemm_bt(q_sk, keys_sk) gives.
//
// LDS (FORGE_SKETCH_TOPK_LDS_BYTES(S) = 128·S + 47744 bytes, 80512 at S = 256:
// two workgroups per CU):
//   q     S/64 chunks of [64 rows × 128 B]: the query tile, staged once
//   ring  3 chunks of [64 slots × 128 B]: the key stream, 2 chunks ahead
//   sc    64 × 68 fp32: one masked score tile (and the final quad merge)
//   meta  4 × 1 KB: ident / stamp / valid of a tile's 64 slots, staged by
//         global_load_lds with the tile's first key chunk
//   qid   64 × i64: the rows' identities, read once per workgroup
//   live  the range's live tiles (u16 offsets), a 512-bit map, their count
// q and ring use gemm_skinny's swizzle (physical = logical ^ ((row & 7) << 4)
// on the 128-byte rows, applied to the global source address when staging and
// to the LDS address when reading fragments).
//
// Pre-pass: a wave per tile ballots "slot < active, valid, stamp >= min_stamp"
// over the tile's 64 slots; tiles with no such slot never enter the stream, so
// a young or idle cache costs no MFMA and no key traffic. The identity is not
// part of this test: it differs per row.
//
// Stream: the chunks (live tile, k-step of 64) form one sequence through the
// ring. Iteration g stages chunk g+2 into the slot chunk g-1 was read from,
// runs chunk g's two K-steps, then retires chunk g+1 with a counted
// `s_waitcnt vmcnt(N)` (N = the loads of chunk g+2: 2, or 3 with a tile's
// metadata load) and one barrier. No score and no metadata passes through a
// register-returning global load inside the loop, so the compiler adds no
// vmcnt(0) of its own.
//
// Epilogue per tile: each lane masks its 2 columns × 8 rows (slot metadata and
// row identities from LDS) to -inf and writes the tile to `sc`; then four
// threads per row (columns q, q+4, ...) each fold 16 scores into a sorted
// 8-entry list in registers. A thread sees slots in ascending order, so
// "insert when strictly greater than the last entry, bubble up while strictly
// greater" keeps the total order (score descending, slot ascending). At the
// end the four lists of a row are merged through `sc` and the first k pairs go
// to partial_*[row, split, 0..k). A top-8 cut to k is the top-k, so k is a
// run-time argument.
//
// ---- sketch_topk_merge_kernel ----
// One wave per row: k rounds, each the wave's best pair that comes after the
// previous pick in the total order (slots are distinct across splits, so the
// order is strict). The result does not depend on `splits`. With n = 0 pairs
// it writes the padding: this is how active == 0 fills out_*.
//
// ---- verify_topk_kernel ----
// One wave per row, four per block. The feature row is loaded once into
// registers (CHUNKS × 8 bf16 per lane) and each candidate's dot runs the
// operations of wave_dot_bf16 in the same order, so a pair's value has the
// bits hip.verify_dot gives. Best of k is a wave-uniform select, first listed
// wins; lane 0 stores.

#include "gemm_common.h"

#define TK_TILE 64
#define TK_ROWB 128
#define TK_CHUNK (TK_TILE * TK_ROWB)        // 8 KB
#define TK_RING 3
#define TK_AHEAD 2
#define TK_SC_STRIDE 68                     // floats; 4·row + col covers the 64 banks
#define TK_SC_BYTES (TK_TILE * TK_SC_STRIDE * 4)
#define TK_META_RING 4
#define TK_META_BYTES 1024                  // ident 512 | stamp 256 | valid 64 (+ 192 unused)
#define TK_KMAX FORGE_SKETCH_TOPK_MAX_K
#define TK_FIXED_BYTES (TK_RING * TK_CHUNK + TK_SC_BYTES + TK_META_RING * TK_META_BYTES + 512 + 1152)
#define TK_NONE (-1e30f)

static_assert(TK_FIXED_BYTES == FORGE_SKETCH_TOPK_LDS_BYTES(0), "LDS layout and forge_api.h disagree");
static_assert(FORGE_SKETCH_TOPK_MAX_TILES == 512, "live list and bitmap hold 512 tiles");
static_assert(TK_KMAX == 8, "lists hold 8 entries");
static_assert(256 * TK_KMAX * 8 <= TK_SC_BYTES, "the quad merge reuses the score tile");

typedef __attribute__((address_space(1))) const void* tk_gptr;
typedef __attribute__((address_space(3))) void* tk_lptr;

__device__ __forceinline__ uint32_t swz_tk(uint32_t byte_off) {
    return byte_off ^ (((byte_off >> 7) & 7u) << 4);
}

// (va, ia) comes before (vb, ib) in the total order (score descending, slot
// ascending); a pair without a slot comes last.
__device__ __forceinline__ bool tk_before(float va, int ia, float vb, int ib) {
    return ia >= 0 && (ib < 0 || va > vb || (va == vb && ia < ib));
}

__device__ __forceinline__ void tk_wait_vm(int n) {
    if (n == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if (n == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// LDS writes of this wave done, then the workgroup barrier
__device__ __forceinline__ void tk_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

__global__ __launch_bounds__(256, 2) void sketch_topk_kernel(
    const short* __restrict__ q_sk,        // [B, S] bf16
    const short* __restrict__ keys_sk,     // [>= n_tiles * 64, S] bf16
    const uint32_t* __restrict__ ident32,  // i64 per slot, as dword pairs
    const uint32_t* __restrict__ stamp,    // unsigned ticks per slot
    const uint8_t* __restrict__ valid,     // 4-byte aligned
    const int64_t* __restrict__ q_ident,   // [B]
    uint32_t min_stamp, int active, int S, int n_tiles, int splits, int k,
    float* __restrict__ partial_val,       // [B, splits, k]
    int32_t* __restrict__ partial_idx)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int n_kt = S / 64;
    char* lds_q = lds;
    char* lds_b = lds + (size_t)n_kt * TK_CHUNK;
    float* sc = (float*)(lds_b + TK_RING * TK_CHUNK);
    char* meta = (char*)sc + TK_SC_BYTES;
    int64_t* qid = (int64_t*)(meta + TK_META_RING * TK_META_BYTES);
    uint16_t* live = (uint16_t*)((char*)qid + 512);
    uint32_t* bm = (uint32_t*)((char*)live + 1024);
    int* n_live_p = (int*)(bm + 16);

    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = tid >> 6;
    const int wm = wave >> 1;
    const int wn = wave & 1;
    const int row_g0 = blockIdx.x * TK_TILE;
    const int split = blockIdx.y;
    const int t0 = (int)((int64_t)split * n_tiles / splits);
    const int t1 = (int)((int64_t)(split + 1) * n_tiles / splits);

    // ---- pre-pass: which tiles of [t0, t1) hold a slot any row could take ----
    if (tid < 16) bm[tid] = 0;
    if (tid < TK_TILE) qid[tid] = q_ident[row_g0 + tid];
    tk_lds_barrier();
    for (int t = t0 + wave; t < t1; t += 4) {
        int c = t * TK_TILE + lane;
        bool ok = false;
        if (c < active) ok = valid[c] != 0 && stamp[c] >= min_stamp;
        uint64_t b = __ballot(ok);
        if (lane == 0 && b) atomicOr(&bm[(t - t0) >> 5], 1u << ((t - t0) & 31));
    }
    tk_lds_barrier();
    if (wave == 0) {
        uint32_t w = lane < 16 ? bm[lane] : 0u;
        int cnt = __popc(w), incl = cnt;
        #pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            int o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        int pos = incl - cnt;
        while (w) {
            int b = __ffs(w) - 1;
            live[pos++] = (uint16_t)(lane * 32 + b);
            w &= w - 1;
        }
        if (lane == WAVE - 1) *n_live_p = incl;
    }
    tk_lds_barrier();
    const int n_live = __builtin_amdgcn_readfirstlane(*n_live_p);

    // this thread's running list: row tid >> 2, columns (tid & 3) + 4j
    float lv[TK_KMAX];
    int li[TK_KMAX];
    #pragma unroll
    for (int j = 0; j < TK_KMAX; ++j) { lv[j] = -INFINITY; li[j] = -1; }

    if (n_live > 0) {
        const int total = n_live * n_kt;

        // ---- the query tile, once: chunk kt is gemm_skinny's A slot of K-tile kt ----
        for (int kt = 0; kt < n_kt; ++kt) {
            #pragma unroll
            for (int i = 0; i < 2; ++i) {
                uint32_t L = swz_tk((uint32_t)(i * 256 + tid) * 16u);
                uint32_t row = L >> 7, colb = L & 127u;
                const short* g = q_sk + ((size_t)(row_g0 + row) * S + kt * 64) + (colb >> 1);
                __builtin_amdgcn_global_load_lds((tk_gptr)g,
                    (tk_lptr)(lds_q + (size_t)kt * TK_CHUNK + (i * 256 + wave * 64) * 16), 16, 0, 0);
            }
        }

        // ---- key stream ----
        int s_T = 0, s_kt = 0, s_slot = 0;     // staging cursor: live ordinal, k-tile, ring slot
        // stages the cursor's chunk and advances; → global_load_lds issued per thread
        auto stage_next = [&]() -> int {
            const int tile = t0 + __builtin_amdgcn_readfirstlane((int)live[s_T]);
            int n_loads = 2;
            #pragma unroll
            for (int i = 0; i < 2; ++i) {
                uint32_t L = swz_tk((uint32_t)(i * 256 + tid) * 16u);
                uint32_t row = L >> 7, colb = L & 127u;
                const short* g = keys_sk + ((size_t)(tile * TK_TILE + row) * S + s_kt * 64) + (colb >> 1);
                __builtin_amdgcn_global_load_lds((tk_gptr)g,
                    (tk_lptr)(lds_b + (size_t)s_slot * TK_CHUNK + (i * 256 + wave * 64) * 16), 16, 0, 0);
            }
            if (s_kt == 0) {
                // one metadata load per wave: ident dwords 0..63, 64..127, stamp, valid
                char* dst = meta + (s_T & (TK_META_RING - 1)) * TK_META_BYTES + wave * 256;
                const size_t c0 = (size_t)tile * TK_TILE;
                if (wave == 3) {
                    // 64 validity bytes as 16 dwords
                    if (lane < 16)
                        __builtin_amdgcn_global_load_lds((tk_gptr)(valid + c0 + lane * 4), (tk_lptr)dst, 4, 0, 0);
                } else {
                    const uint32_t* g = wave == 2 ? stamp + c0 + lane : ident32 + c0 * 2 + wave * 64 + lane;
                    __builtin_amdgcn_global_load_lds((tk_gptr)g, (tk_lptr)dst, 4, 0, 0);
                }
                n_loads = 3;
            }
            if (++s_kt == n_kt) { s_kt = 0; ++s_T; }
            s_slot = s_slot == TK_RING - 1 ? 0 : s_slot + 1;
            return n_loads;
        };

        int newest = 0;                         // loads of the newest staged chunk
        #pragma unroll
        for (int g = 0; g < TK_AHEAD; ++g)
            if (g < total) newest = stage_next();
        tk_wait_vm(total > 1 ? newest : 0);     // retires the query tile and chunk 0
        __builtin_amdgcn_s_barrier();

        f32x4 acc[2][2];
        const uint32_t k_col = (uint32_t)((lane >> 4) * 16);
        const uint32_t a_row_base = (uint32_t)(wm * 32 + (lane & 15));
        const uint32_t b_row_base = (uint32_t)(wn * 32 + (lane & 15));
        int c_T = 0, c_kt = 0, c_slot = 0;      // compute cursor

        for (int g = 0; g < total; ++g) {
            int staged = 0;
            if (g + TK_AHEAD < total) staged = stage_next();
            if (c_kt == 0) {
                #pragma unroll
                for (int i = 0; i < 2; ++i)
                    #pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            const char* slot_a = lds_q + (size_t)c_kt * TK_CHUNK;
            const char* slot_b = lds_b + (size_t)c_slot * TK_CHUNK;
            #pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 a_frag[2], b_frag[2];
                #pragma unroll
                for (int f = 0; f < 2; ++f) {
                    uint32_t ra = a_row_base + f * 16, rb = b_row_base + f * 16;
                    a_frag[f] = *(const bf16x8*)(slot_a + swz_tk(ra * TK_ROWB + kk * 64 + k_col));
                    b_frag[f] = *(const bf16x8*)(slot_b + swz_tk(rb * TK_ROWB + kk * 64 + k_col));
                }
                #pragma unroll
                for (int fr = 0; fr < 2; ++fr)
                    #pragma unroll
                    for (int fc = 0; fc < 2; ++fc)
                        acc[fr][fc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag[fr], b_frag[fc], acc[fr][fc], 0, 0, 0);
            }
            // chunk boundary: retire chunk g+1, the chunk staged above stays in flight
            tk_wait_vm(staged);
            tk_lds_barrier();

            if (c_kt == n_kt - 1) {
                // ---- epilogue of live tile c_T ----
                const int c0 = (t0 + __builtin_amdgcn_readfirstlane((int)live[c_T])) * TK_TILE;
                const char* me = meta + (c_T & (TK_META_RING - 1)) * TK_META_BYTES;
                #pragma unroll
                for (int fc = 0; fc < 2; ++fc) {
                    const int col = wn * 32 + fc * 16 + (lane & 15);
                    const int64_t sid = *(const int64_t*)(me + col * 8);
                    const uint32_t st = *(const uint32_t*)(me + 512 + col * 4);
                    const uint8_t vd = *(const uint8_t*)(me + 768 + col);
                    const bool ok = (c0 + col < active) && vd != 0 && st >= min_stamp;
                    #pragma unroll
                    for (int fr = 0; fr < 2; ++fr) {
                        const int r0 = wm * 32 + fr * 16 + (lane >> 4) * 4;
                        #pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const bool take = ok && qid[r0 + reg] == sid;
                            sc[(r0 + reg) * TK_SC_STRIDE + col] = take ? acc[fr][fc][reg] : -INFINITY;
                        }
                    }
                }
                tk_lds_barrier();
                const float* srow = sc + (tid >> 2) * TK_SC_STRIDE + (tid & 3);
                #pragma unroll
                for (int j = 0; j < TK_TILE / 4; ++j) {
                    const float v = srow[j * 4];
                    if (v > lv[TK_KMAX - 1]) {
                        lv[TK_KMAX - 1] = v;
                        li[TK_KMAX - 1] = c0 + j * 4 + (tid & 3);
                        #pragma unroll
                        for (int p = TK_KMAX - 1; p > 0; --p) {
                            if (lv[p] > lv[p - 1]) {
                                float tv = lv[p]; lv[p] = lv[p - 1]; lv[p - 1] = tv;
                                int ti = li[p]; li[p] = li[p - 1]; li[p - 1] = ti;
                            }
                        }
                    }
                }
                c_kt = 0;
                ++c_T;
            } else {
                ++c_kt;
            }
            c_slot = c_slot == TK_RING - 1 ? 0 : c_slot + 1;
        }
        tk_lds_barrier();   // every thread is done with the last score tile
    }

    // ---- merge the four lists of a row, write the split's k pairs ----
    float* fv = sc;
    int* fi = (int*)sc + 256 * TK_KMAX;
    #pragma unroll
    for (int j = 0; j < TK_KMAX; ++j) { fv[tid * TK_KMAX + j] = lv[j]; fi[tid * TK_KMAX + j] = li[j]; }
    tk_lds_barrier();
    if ((tid & 3) == 0) {
        const size_t out0 = ((size_t)(row_g0 + (tid >> 2)) * splits + split) * k;
        uint32_t heads = 0;                     // a nibble per list
        for (int o = 0; o < k; ++o) {
            float bv = 0.f;
            int bi = -1, bq = 0;
            #pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int h = (heads >> (4 * q)) & 15;
                if (h < TK_KMAX) {
                    const float v = fv[(tid + q) * TK_KMAX + h];
                    const int i = fi[(tid + q) * TK_KMAX + h];
                    if (tk_before(v, i, bv, bi)) { bv = v; bi = i; bq = q; }
                }
            }
            if (bi >= 0) heads += 1u << (4 * bq);
            partial_val[out0 + o] = bi >= 0 ? bv : TK_NONE;
            partial_idx[out0 + o] = bi;
        }
    }
}

__global__ __launch_bounds__(256) void sketch_topk_merge_kernel(
    const float* __restrict__ partial_val, const int32_t* __restrict__ partial_idx,
    int B, int n, int k,                   // n = splits * k pairs per row
    float* __restrict__ out_val, int32_t* __restrict__ out_idx)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (row >= B) return;
    const float* pv = partial_val + (size_t)row * n;
    const int32_t* pi = partial_idx + (size_t)row * n;
    float prev_v = 0.f;
    int prev_i = -1;
    for (int o = 0; o < k; ++o) {
        float bv = 0.f;
        int bi = -1;
        for (int p = lane; p < n; p += WAVE) {
            const float v = pv[p];
            const int i = pi[p];
            if ((o == 0 || tk_before(prev_v, prev_i, v, i)) && tk_before(v, i, bv, bi)) { bv = v; bi = i; }
        }
        #pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (tk_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        prev_v = bv;
        prev_i = bi;
        if (lane == 0) {
            out_val[(size_t)row * k + o] = bi >= 0 ? bv : TK_NONE;
            out_idx[(size_t)row * k + o] = bi;
        }
    }
}

extern "C" int forge_sketch_topk(
    const void* q_sk, const void* keys_sk, const void* ident, const void* stamp, const void* valid,
    const void* q_ident, uint32_t min_stamp, int active, int B, int S, int k, int splits,
    void* partial_val, void* partial_idx, void* out_val, void* out_idx, void* stream)
{
    if (k < 1 || k > FORGE_SKETCH_TOPK_MAX_K) return FORGE_ERR_SEMCACHE_TOPK;
    if (S < 64 || S > 512 || (S % 64)) return FORGE_ERR_SEMCACHE_TOPK;
    if (B < 0 || (B % TK_TILE) || active < 0) return FORGE_ERR_SEMCACHE_TOPK;
    if (splits < 0 || splits > FORGE_SKETCH_TOPK_MAX_SPLITS) return FORGE_ERR_SEMCACHE_TOPK;
    if (B == 0) return 0;
    if (out_val == nullptr || out_idx == nullptr) return FORGE_ERR_SEMCACHE_TOPK;
    const int n_tiles = ceil_div(active, TK_TILE);
    const int min_splits = ceil_div(n_tiles, FORGE_SKETCH_TOPK_MAX_TILES);
    if (min_splits > FORGE_SKETCH_TOPK_MAX_SPLITS || (splits > 0 && splits < min_splits)) return FORGE_ERR_SEMCACHE_TOPK;
    if (active > 0 && (partial_val == nullptr || partial_idx == nullptr)) return FORGE_ERR_SEMCACHE_TOPK;
    hipStream_t s = (hipStream_t)stream;
    const int row_tiles = B / TK_TILE;
    if (active == 0) {
        // nothing to sweep: the merge kernel over zero pairs writes the padding
        splits = 0;
    } else {
        if (splits == 0) {
            splits = ceil_div(FORGE_SKETCH_TOPK_TARGET_BLOCKS, row_tiles);
            if (splits > n_tiles) splits = n_tiles;
            if (splits > FORGE_SKETCH_TOPK_MAX_SPLITS) splits = FORGE_SKETCH_TOPK_MAX_SPLITS;
            if (splits < min_splits) splits = min_splits;
        }
        const int lds_bytes = FORGE_SKETCH_TOPK_LDS_BYTES(S);
        hipError_t e = hipFuncSetAttribute((const void*)sketch_topk_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(sketch_topk_kernel, dim3(row_tiles, splits), dim3(256), lds_bytes, s,
                           (const short*)q_sk, (const short*)keys_sk, (const uint32_t*)ident,
                           (const uint32_t*)stamp, (const uint8_t*)valid, (const int64_t*)q_ident,
                           min_stamp, active, S, n_tiles, splits, k,
                           (float*)partial_val, (int32_t*)partial_idx);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(sketch_topk_merge_kernel, dim3(ceil_div(B, ROW_WAVES)), dim3(256), 0, s,
                       (const float*)partial_val, (const int32_t*)partial_idx, B, splits * k, k,
                       (float*)out_val, (int32_t*)out_idx);
    return (int)hipGetLastError();
}

// CHUNKS × 512 >= D: the feature row in registers, 8 bf16 per lane and chunk.
template <int CHUNKS>
__global__ __launch_bounds__(256) void verify_topk_kernel(
    const short* __restrict__ feats,   // [M, D] bf16
    const short* __restrict__ keys,    // [capacity, D] bf16
    const int32_t* __restrict__ cand,  // [M, k] slots, -1 = none
    int k, int M, int D,
    float* __restrict__ best_val, int32_t* __restrict__ best_idx)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int r = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (r >= M) return;
    short8 a[CHUNKS];
    #pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
        const int kx = lane * 8 + c * WAVE * 8;
        a[c] = kx < D ? *(const short8*)(feats + (size_t)r * D + kx) : (short8){0, 0, 0, 0, 0, 0, 0, 0};
    }
    float bv = TK_NONE;
    int bi = -1;
    for (int j = 0; j < k; ++j) {
        const int slot = __builtin_amdgcn_readfirstlane(cand[(size_t)r * k + j]);
        if (slot < 0) continue;
        const short* b_row = keys + (size_t)slot * D;
        // wave_dot_bf16 with the a row held in registers: same chunks, same order
        float dot = 0.0f;
        #pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const int kx = lane * 8 + c * WAVE * 8;
            if (kx < D) {
                short8 bvec = *(const short8*)(b_row + kx);
                #pragma unroll
                for (int e = 0; e < 8; ++e) dot += bf16_to_f(a[c][e]) * bf16_to_f(bvec[e]);
            }
        }
        const float v = __shfl(wave_sum(dot), 0);
        if (bi < 0 || v > bv) { bv = v; bi = slot; }
    }
    if (lane == 0) { best_val[r] = bv; best_idx[r] = bi; }
}

extern "C" int forge_verify_topk(
    const void* feats, const void* keys, const void* cand, int k, int M, int D,
    void* best_val, void* best_idx, void* stream)
{
    if (D % 8) return FORGE_ERR_ROW_ALIGN;
    if (k < 1 || k > FORGE_SKETCH_TOPK_MAX_K || D <= 0 || D > FORGE_VERIFY_TOPK_MAX_D) return FORGE_ERR_SEMCACHE_TOPK;
    if (M <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(ceil_div(M, ROW_WAVES));
    #define LAUNCH_VERIFY(CH) \
        hipLaunchKernelGGL(verify_topk_kernel<CH>, grid, dim3(256), 0, s, (const short*)feats, (const short*)keys, \
                           (const int32_t*)cand, k, M, D, (float*)best_val, (int32_t*)best_idx)
    if (D <= 512) LAUNCH_VERIFY(1);
    else if (D <= 4096) LAUNCH_VERIFY(8);
    else LAUNCH_VERIFY(16);
    #undef LAUNCH_VERIFY
    return (int)hipGetLastError();
}
