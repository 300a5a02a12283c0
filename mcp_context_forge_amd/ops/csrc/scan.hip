// Multi-pattern DFA scan over a packed request batch.
//
// Tables come from ops/dfa.py (compile_patterns); semantics are identical to
// dfa.scan_reference / match_mask_reference — the CPU oracle in tests.
// Reference-gateway analog: the per-request regex/deny/PII/harm scans
// (plugins/deny_filter, regex_filter, cpex-pii-filter,
// harmful_content_detector) executed per request in Python `re`; here one
// kernel scans the whole micro-batch.
//
// Parallelization: one thread per request (requests are short JSON payloads,
// ~100 B–4 KB). The transition table is small (tens of KB) and L2/LDS-
// resident. When the table fits in 64 KB of LDS the block cooperatively
// stages it (fast path); otherwise lanes read it through L2.

#include "common.h"

#include <stddef.h>

struct ScanTables {
    const uint16_t* next;    // [S, C]
    const uint8_t* klass;    // [256]
    const uint32_t* accept;  // [S]
};

// Block-cooperative copy of one bank's tables into LDS; returns the LDS
// copies. The layout (next, klass, accept back to back) is what
// FORGE_SCAN_TABLE_BYTES sizes. Every thread of the block must call it.
__device__ __forceinline__ ScanTables stage_tables_lds(
    uint8_t* lds_raw, const ScanTables& g, int n_states, int n_classes)
{
    uint16_t* lnext = (uint16_t*)lds_raw;
    uint8_t* lklass = (uint8_t*)(lds_raw + (size_t)n_states * n_classes * 2);
    uint32_t* laccept = (uint32_t*)(lklass + 256);
    int total16 = n_states * n_classes;
    for (int i = threadIdx.x; i < total16; i += blockDim.x) lnext[i] = g.next[i];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) lklass[i] = g.klass[i];
    for (int i = threadIdx.x; i < n_states; i += blockDim.x) laccept[i] = g.accept[i];
    __syncthreads();
    return ScanTables{lnext, lklass, laccept};
}

template <bool USE_LDS>
__global__ __launch_bounds__(256) void scan_kernel(
    const uint8_t* __restrict__ data,     // packed bytes
    const int32_t* __restrict__ beg,
    const int32_t* __restrict__ end_,
    int batch,
    const uint16_t* __restrict__ next,    // [S, C]
    const uint8_t* __restrict__ klass,    // [256]
    const uint32_t* __restrict__ accept,  // [S]
    int n_states, int n_classes,
    uint32_t* __restrict__ out_mask,      // [B] pattern-id bitmask
    int32_t* __restrict__ out_first_end)  // [B] first match end (or -1); optional
{
    extern __shared__ uint8_t lds_raw[];
    ScanTables t{next, klass, accept};
    if constexpr (USE_LDS) t = stage_tables_lds(lds_raw, t, n_states, n_classes);

    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= batch) return;
    int32_t rbeg = beg[r], rend = end_[r];
    uint32_t mask = 0;
    int32_t first_end = -1;
    uint32_t state = 0;
    for (int32_t p = rbeg; p < rend; ++p) {
        uint8_t b = data[p];
        state = t.next[state * n_classes + t.klass[b]];
        uint32_t a = t.accept[state];
        if (a) {
            if (first_end < 0) first_end = p + 1 - rbeg;
            mask |= a;
        }
    }
    out_mask[r] = mask;
    if (out_first_end) out_first_end[r] = first_end;
}

// ---------------------------------------------------------------------------
// Fused multi-bank scan: ALL DFA banks in ONE launch (grid.y = bank).
//
// Measured motivation (profiles/README_r02.md stage budget): at HTTP batch
// sizes (~1-3k rows) the per-bank launches + per-bank D2H copies dominate
// the scan stage — six launches of ~128 waves each also underfill 256 CUs.
// One launch with grid (rows/256, n_banks) fills the chip bank-parallel,
// writes one [n_banks, B] mask matrix, and the host does ONE D2H.
//
// Bank descriptors live in device memory (built once per bank-set); each
// block stages ITS bank's table into LDS when it fits the per-block
// allocation (banks over the limit read through L2, same as scan_kernel).

struct ScanBankDesc {
    const uint16_t* next;
    const uint8_t* klass;
    const uint32_t* accept;
    int n_states;
    int n_classes;
    int use_lds;   // table fits the dynamic LDS allocation
    int _pad[3];
};
// ops/hip.py ScanBankSet packs each descriptor as six little-endian int64:
// [next, klass, accept, n_states | n_classes << 32, use_lds, 0].
static_assert(sizeof(ScanBankDesc) == 6 * sizeof(int64_t), "ScanBankDesc is six int64");
static_assert(offsetof(ScanBankDesc, next) == 0 && offsetof(ScanBankDesc, klass) == 8 &&
              offsetof(ScanBankDesc, accept) == 16 && offsetof(ScanBankDesc, n_states) == 24 &&
              offsetof(ScanBankDesc, n_classes) == 28 && offsetof(ScanBankDesc, use_lds) == 32,
              "ScanBankDesc field offsets must match ScanBankSet's packing");

__global__ __launch_bounds__(256) void scan_multi_kernel(
    const uint8_t* __restrict__ data,
    const int32_t* __restrict__ beg,
    const int32_t* __restrict__ end_,
    int batch,
    const ScanBankDesc* __restrict__ descs,
    uint32_t* __restrict__ out_mask)      // [n_banks, batch]
{
    extern __shared__ uint8_t lds_raw[];
    const ScanBankDesc d = descs[blockIdx.y];
    ScanTables t{d.next, d.klass, d.accept};
    if (d.use_lds) t = stage_tables_lds(lds_raw, t, d.n_states, d.n_classes);
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= batch) return;
    int32_t rbeg = beg[r], rend = end_[r];
    uint32_t mask = 0;
    uint32_t state = 0;
    int nc = d.n_classes;
    for (int32_t p = rbeg; p < rend; ++p) {
        state = t.next[state * nc + t.klass[data[p]]];
        mask |= t.accept[state];
    }
    out_mask[(size_t)blockIdx.y * batch + r] = mask;
}

extern "C" int forge_scan_multi(
    const void* data, const void* beg, const void* end_, int batch,
    const void* descs_dev, int n_banks, int lds_bytes,
    void* out_mask, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    int block = 256;
    dim3 grid((unsigned)ceil_div(batch, block), (unsigned)n_banks);
    hipLaunchKernelGGL(scan_multi_kernel, grid, dim3(block), (size_t)lds_bytes, s,
                       (const uint8_t*)data, (const int32_t*)beg, (const int32_t*)end_, batch,
                       (const ScanBankDesc*)descs_dev, (uint32_t*)out_mask);
    return (int)hipGetLastError();
}

extern "C" int forge_scan(
    const void* data, const void* beg, const void* end_, int batch,
    const void* next, const void* klass, const void* accept,
    int n_states, int n_classes,
    void* out_mask, void* out_first_end, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    int block = 256;
    int grid = ceil_div(batch, block);
    size_t table_bytes = (size_t)FORGE_SCAN_TABLE_BYTES(n_states, n_classes);
    if (table_bytes <= FORGE_SCAN_LDS_LIMIT) {
        hipLaunchKernelGGL((scan_kernel<true>), dim3(grid), dim3(block), table_bytes, s,
                           (const uint8_t*)data, (const int32_t*)beg, (const int32_t*)end_, batch,
                           (const uint16_t*)next, (const uint8_t*)klass, (const uint32_t*)accept,
                           n_states, n_classes, (uint32_t*)out_mask, (int32_t*)out_first_end);
    } else {
        hipLaunchKernelGGL((scan_kernel<false>), dim3(grid), dim3(block), 0, s,
                           (const uint8_t*)data, (const int32_t*)beg, (const int32_t*)end_, batch,
                           (const uint16_t*)next, (const uint8_t*)klass, (const uint32_t*)accept,
                           n_states, n_classes, (uint32_t*)out_mask, (int32_t*)out_first_end);
    }
    return (int)hipGetLastError();
}
