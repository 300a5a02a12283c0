// Per-request JSON structure walk against compiled tool schemas: the kernel
// half of schema_guard for the schemas its byte patterns cannot hold.
//
// "Is this depth-1 key one of the tool's properties, is its value of the right
// type, inside its enum, its bound, its length, and is any required key
// missing" needs keys told from values, depth 1 from deeper, an integer's value
// from its digits. The search-semantics DFA banks of scan.hip can hold none of
// it. Semantics are identical to ops/schema.py schema_check_reference, whose
// docstring is the definition; the kernel says PASS only where
// utils/jsonschema.validate would, and everything else takes the host path.
//
// Parallelization: one wavefront per request, as url.hip and unicode.hip. The
// hash powers (64 x u32), the powers of ten (9 x u32) and, when they fit, the
// tool and property records are put into LDS once per block. Then lane p takes
// property p of the request's tool into registers: a tool has at most 64, so
// the whole lookup table of a request is one record per lane.
//
// Structure, 64 bytes a step from the span's begin (one per lane, zero past
// the end): string membership is the prefix XOR of the quote ballot with one
// carried bit; the depth at a lane is the carried depth plus the popcounts of
// the open and close ballots up to it; '{' that reaches depth 1 and ',' ':' at
// depth 1 are three more ballots. An opening quote at depth 1 whose nearest
// structural bit below it (or the carried one) is '{' or ',' starts a key. A
// chunk without one costs its ballots and nothing else, and so do bytes at
// depth >= 2.
//
// Keys are walked with ctz, the whole wave on one key, by absolute position,
// so a key, a colon or a value may lie in any later chunk:
//   * closing quote: ballots over the 65 bytes after the opening one;
//   * lookup: lane i forms c_i * B^(L-1-i), a butterfly sum gives the hash in
//     every lane, one ballot against the lanes' records gives the candidates,
//     and a candidate's pool bytes are compared one per lane, so a hash
//     collision cannot change a result;
//   * the record of the property found moves to every lane by lane reads;
//   * colon, value start, token end, closing quote of a string value: ballot
//     searches in 64-byte steps, so a string under a length bound may be long;
//   * integer: lane i holds digit i times 10^(r mod 9), r its place from the
//     right; two butterfly sums give the low and the high nine digits;
//   * enum: entries 64 at a time, one per lane; a string entry is matched by
//     hash and length and then byte-compared like a key.
//
// All control flow derives from ballots, lane reads and kernel arguments, so
// every branch but the record loads is wave-uniform. Lane 0 writes the four
// outputs of every request.

#include <stddef.h>

#include "common.h"

struct SchemaTool {
    uint32_t prop_beg, prop_cnt, flags, pad;
    uint64_t required;
};
struct SchemaProp {
    uint32_t key_hash, key_off, key_len, tflags;
    int64_t lo, hi;
    uint32_t enum_beg, enum_cnt;
};
struct SchemaEnum {
    int64_t value;   // of an integer entry; the hash of a string entry
    uint32_t off, len;
};
static_assert(sizeof(SchemaTool) == FORGE_SCHEMA_TOOL_BYTES && offsetof(SchemaTool, required) == 16,
              "SchemaTool is <IIIIQ in ops/schema.py");
static_assert(sizeof(SchemaProp) == FORGE_SCHEMA_PROP_BYTES && offsetof(SchemaProp, lo) == 16 &&
              offsetof(SchemaProp, enum_beg) == 32, "SchemaProp is <IIIIqqII in ops/schema.py");
static_assert(sizeof(SchemaEnum) == FORGE_SCHEMA_ENUM_BYTES && offsetof(SchemaEnum, off) == 8,
              "SchemaEnum is <qII in ops/schema.py");

#define SCH_B 0x01000193u   // ops/schema.py HASH_B
#define SCH_MAX_KEY 64
#define SCH_MAX_DIGITS 18
#define SCH_POW_BYTES ((WAVE + 16) * 4)   // hash powers, then nine powers of ten
static_assert(SCH_POW_BYTES % 8 == 0 && (FORGE_SCHEMA_LDS_TOOLS * FORGE_SCHEMA_TOOL_BYTES) % 8 == 0, "records are 8-aligned");
static_assert(SCH_POW_BYTES + FORGE_SCHEMA_LDS_TOOLS * FORGE_SCHEMA_TOOL_BYTES +
              FORGE_SCHEMA_LDS_PROPS * FORGE_SCHEMA_PROP_BYTES <= 16 * 1024, "16 KiB of LDS at most");
static_assert(FORGE_SCHEMA_MAX_TOOL_PROPS == WAVE, "one property per lane");

enum { SCH_T_STRING = 1, SCH_T_INTEGER = 2, SCH_T_NUMBER = 4, SCH_T_BOOLEAN = 8, SCH_T_NULL = 16, SCH_T_OBJECT = 32,
       SCH_T_ARRAY = 64, SCH_F_BOUND = 0x100, SCH_F_LENGTH = 0x200, SCH_F_ENUM = 0x400 };
enum { SCH_COMPILED = 1, SCH_NO_ADDITIONAL = 2 };
enum { SCH_PASS = 0, SCH_FAIL = 1, SCH_PUNT = 2 };
enum { SCH_MISSING = 1, SCH_TYPE = 2, SCH_ENUM = 4, SCH_BOUND = 8, SCH_LENGTH = 16, SCH_ADDITIONAL = 32 };
enum { SCH_BACKSLASH = 1, SCH_NON_ASCII = 2, SCH_NOT_OBJECT = 4, SCH_LONG = 8, SCH_DUP_KEY = 16, SCH_NUMBER_FORM = 32,
       SCH_NO_TABLE = 64 };
enum { SCH_QUOTE, SCH_COLON, SCH_NONWS, SCH_TOKEND };

__device__ __forceinline__ bool sch_ws(uint32_t b) { return b == ' ' || b == '\t' || b == '\n' || b == '\r'; }

// the sum over the wave, in every lane
__device__ __forceinline__ uint32_t sch_sum(uint32_t v) {
    #pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t other = __shfl_xor(v, off);
        v += other;
    }
    return v;
}

// lane `src`'s value, in every lane
__device__ __forceinline__ int64_t sch_lane64(int64_t v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src);
    const uint32_t hi = __shfl((uint32_t)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The first position in [p, lim) whose byte is of KIND, or lim. Reads no byte outside [p, lim).
template <int KIND>
__device__ __forceinline__ int32_t sch_find(const uint8_t* __restrict__ data, int32_t p, int32_t lim, int lane) {
    for (int64_t q = p; q < lim; q += WAVE) {
        const bool in = lane < lim - q;
        const uint32_t b = in ? data[q + lane] : 0u;
        const bool hit = KIND == SCH_QUOTE ? b == '"' : KIND == SCH_COLON ? b == ':' : KIND == SCH_NONWS ? !sch_ws(b)
                       : (sch_ws(b) || b == ',' || b == '}');
        const uint64_t m = __ballot(in && hit);
        if (m) return (int32_t)q + __builtin_ctzll(m);
    }
    return lim;
}

// hash of the `len` <= 64 bytes the lanes below `len` hold, in every lane
__device__ __forceinline__ uint32_t sch_hash(uint32_t c, int len, int lane, const uint32_t* lpow) {
    return sch_sum(lane < len ? c * lpow[len - 1 - lane] : 0u);
}

// do the `len` bytes the lanes hold equal pool[off, off + len)?
__device__ __forceinline__ bool sch_same(const uint8_t* __restrict__ pool, uint32_t off, uint32_t c, int len, int lane) {
    const uint32_t pc = lane < len ? pool[(size_t)off + lane] : 0u;
    return __ballot(lane < len && pc != c) == 0ull;
}

struct SchState {
    uint32_t fail, punt;
    uint64_t seen;
};

// Judge the key whose opening quote stands at q (rules 5 to 8 of the reference).
__device__ __forceinline__ void sch_key(
    const uint8_t* __restrict__ data, int32_t q, int32_t rend, int lane,
    const uint32_t* lpow, const uint32_t* lp10, const SchemaProp& pr, int n_props, uint32_t tool_flags,
    const SchemaEnum* __restrict__ enums, const uint8_t* __restrict__ pool, SchState& st)
{
    const int32_t ks = q + 1;
    const int32_t klim = rend - ks > SCH_MAX_KEY + 1 ? ks + SCH_MAX_KEY + 1 : rend;
    const int32_t ke = sch_find<SCH_QUOTE>(data, ks, klim, lane);
    if (ke == klim) {
        st.punt = SCH_LONG;
        return;
    }
    const int klen = ke - ks;   // 0..64
    const uint32_t kc = lane < klen ? data[(int64_t)ks + lane] : 0u;
    const uint32_t kh = sch_hash(kc, klen, lane, lpow);
    uint64_t cand = __ballot(lane < n_props && pr.key_hash == kh && pr.key_len == (uint32_t)klen);
    int pi = -1;
    while (cand && pi < 0) {
        const int t = __builtin_ctzll(cand);
        cand &= cand - 1ull;
        const uint32_t off = __shfl(pr.key_off, t);
        if (sch_same(pool, off, kc, klen, lane)) pi = t;
    }
    if (pi < 0) {
        if (tool_flags & SCH_NO_ADDITIONAL) st.fail |= SCH_ADDITIONAL;
        return;
    }
    if ((st.seen >> pi) & 1ull) {
        st.punt = SCH_DUP_KEY;
        return;
    }
    st.seen |= 1ull << pi;
    const uint32_t tflags = __shfl(pr.tflags, pi);
    const int64_t lo = sch_lane64(pr.lo, pi), hi = sch_lane64(pr.hi, pi);
    const uint32_t ebeg = __shfl(pr.enum_beg, pi), ecnt = __shfl(pr.enum_cnt, pi);

    const int32_t colon = sch_find<SCH_COLON>(data, ke + 1, rend, lane);
    const int32_t v = sch_find<SCH_NONWS>(data, colon < rend ? colon + 1 : rend, rend, lane);
    if (v == rend) {
        st.punt = SCH_NUMBER_FORM;
        return;
    }
    const uint32_t vb = (lane < 2 && lane < rend - v) ? data[(int64_t)v + lane] : 0u;
    const uint32_t c0 = __shfl(vb, 0), c1 = __shfl(vb, 1);

    uint32_t cls;
    bool has_val = false;
    int64_t val = 0;
    int32_t vs = 0, slen = 0;
    if (c0 == '"') {
        cls = SCH_T_STRING;
        vs = v + 1;
        slen = sch_find<SCH_QUOTE>(data, vs, rend, lane) - vs;
    } else if (c0 == '{' || c0 == '[') {
        cls = c0 == '{' ? SCH_T_OBJECT : SCH_T_ARRAY;
    } else if (c0 == 't' || c0 == 'f' || c0 == 'n') {
        cls = c0 == 'n' ? SCH_T_NULL : SCH_T_BOOLEAN;
    } else if (c0 - '0' < 10u || (c0 == '-' && c1 - '0' < 10u)) {
        const int32_t tlim = rend - v > SCH_MAX_KEY + 1 ? v + SCH_MAX_KEY + 1 : rend;
        const int tlen = sch_find<SCH_TOKEND>(data, v, tlim, lane) - v;
        if (tlen > SCH_MAX_KEY) {
            st.punt = SCH_LONG;
            return;
        }
        const uint32_t w = lane < tlen ? data[(int64_t)v + lane] : 0u;
        if (__ballot(w == '.' || w == 'e' || w == 'E')) {
            cls = SCH_T_NUMBER;
            if (tflags & SCH_F_BOUND) {
                st.punt = SCH_NUMBER_FORM;
                return;
            }
        } else {
            const int neg = c0 == '-' ? 1 : 0;
            const bool in = lane >= neg && lane < tlen;
            if (__ballot(in && w - '0' >= 10u)) {
                st.punt = SCH_NUMBER_FORM;
                return;
            }
            if (tlen - neg > SCH_MAX_DIGITS) {
                st.punt = SCH_LONG;
                return;
            }
            // place r from the right, 0..17: the low nine digits and the high nine are a u32 each
            const int r = in ? tlen - 1 - lane : 0;
            const uint32_t term = in ? (w - '0') * lp10[r < 9 ? r : r - 9] : 0u;
            const uint32_t low = sch_sum(r < 9 ? term : 0u);
            const uint32_t high = sch_sum(r < 9 ? 0u : term);
            val = (int64_t)high * 1000000000ll + (int64_t)low;
            val = neg ? -val : val;
            has_val = true;
            cls = SCH_T_INTEGER | SCH_T_NUMBER;
        }
    } else {
        st.punt = SCH_NUMBER_FORM;
        return;
    }

    if (!(cls & tflags)) {
        st.fail |= SCH_TYPE;
        return;
    }
    if (tflags & SCH_F_ENUM) {
        bool ok = false;
        if (cls == SCH_T_STRING) {
            if (slen <= SCH_MAX_KEY) {
                const uint32_t sc = lane < slen ? data[(int64_t)vs + lane] : 0u;
                const uint32_t sh = sch_hash(sc, slen, lane, lpow);
                for (uint32_t g = 0; g < ecnt && !ok; g += WAVE) {
                    const bool in = g + lane < ecnt;
                    SchemaEnum e = {0, 0u, 0u};
                    if (in) e = enums[(size_t)ebeg + g + lane];
                    uint64_t ec = __ballot(in && (uint32_t)e.value == sh && e.len == (uint32_t)slen);
                    while (ec && !ok) {
                        const int t = __builtin_ctzll(ec);
                        ec &= ec - 1ull;
                        const uint32_t off = __shfl(e.off, t);
                        ok = sch_same(pool, off, sc, slen, lane);
                    }
                }
            }
        } else {
            for (uint32_t g = 0; g < ecnt && !ok; g += WAVE) {
                const bool in = g + lane < ecnt;
                int64_t ev = 0;
                if (in) ev = enums[(size_t)ebeg + g + lane].value;
                ok = __ballot(in && has_val && ev == val) != 0ull;
            }
        }
        if (!ok) st.fail |= SCH_ENUM;
    }
    if ((tflags & SCH_F_BOUND) && has_val && (val < lo || val > hi)) st.fail |= SCH_BOUND;
    if ((tflags & SCH_F_LENGTH) && cls == SCH_T_STRING && (slen < lo || slen > hi)) st.fail |= SCH_LENGTH;
}

__global__ __launch_bounds__(ROW_WAVES * WAVE) void schema_check_kernel(
    const uint8_t* __restrict__ data,    // packed bytes
    const int32_t* __restrict__ beg,
    const int32_t* __restrict__ end_,
    const int32_t* __restrict__ tool_idx,
    int batch,
    const SchemaTool* __restrict__ tools, int n_tools,
    const SchemaProp* __restrict__ props, int n_props,
    int in_lds,
    const SchemaEnum* __restrict__ enums,
    const uint8_t* __restrict__ pool,
    int32_t* __restrict__ out_verdict,   // [B] 0 PASS, 1 FAIL, 2 PUNT
    int32_t* __restrict__ out_fail,      // [B]
    int32_t* __restrict__ out_punt,      // [B]
    uint64_t* __restrict__ out_seen)     // [B]
{
    // powers u32[64], tens u32[16] | tools [LDS_TOOLS] | props [n_props] (the last two when staged)
    extern __shared__ __align__(16) uint8_t lds_raw[];
    uint32_t* lpow = (uint32_t*)lds_raw;
    uint32_t* lp10 = lpow + WAVE;
    SchemaTool* ltools = (SchemaTool*)(lds_raw + SCH_POW_BYTES);
    SchemaProp* lprops = (SchemaProp*)(lds_raw + SCH_POW_BYTES + FORGE_SCHEMA_LDS_TOOLS * FORGE_SCHEMA_TOOL_BYTES);
    if (threadIdx.x < WAVE + 9) {
        // base^i by squaring: thread i < 64 the hash power, thread 64 + i the power of ten
        const bool ten = threadIdx.x >= WAVE;
        uint32_t i = ten ? threadIdx.x - WAVE : threadIdx.x, base = ten ? 10u : SCH_B, p = 1u;
        for (; i; i >>= 1, base *= base) p = (i & 1u) ? p * base : p;
        lpow[threadIdx.x] = p;
    }
    if (in_lds) {
        for (int i = threadIdx.x; i < n_tools; i += blockDim.x) ltools[i] = tools[i];
        for (int i = threadIdx.x; i < n_props; i += blockDim.x) lprops[i] = props[i];
    }
    // every wave of the block reaches this barrier before any wave leaves
    __syncthreads();

    const int lane = threadIdx.x & (WAVE - 1);
    const int r = blockIdx.x * ROW_WAVES + (threadIdx.x / WAVE);
    if (r >= batch) return;  // wave-uniform
    const int32_t rbeg = beg[r], rend = end_[r];
    const int32_t ti = tool_idx[r];

    SchemaTool tl = {0u, 0u, 0u, 0u, 0ull};
    if (ti >= 0 && ti < n_tools) {
        if (in_lds) tl = ltools[ti];
        else tl = tools[ti];
    }
    if (!(tl.flags & SCH_COMPILED)) {
        if (lane == 0) {
            out_verdict[r] = SCH_PUNT;
            out_fail[r] = 0;
            out_punt[r] = SCH_NO_TABLE;
            out_seen[r] = 0ull;
        }
        return;
    }
    // lane p holds property p of the tool
    const int n_tp = (int)tl.prop_cnt;
    SchemaProp pr = {0u, 0u, 0u, 0u, 0ll, 0ll, 0u, 0u};
    if (lane < n_tp) {
        if (in_lds) pr = lprops[tl.prop_beg + lane];
        else pr = props[(size_t)tl.prop_beg + lane];
    }

    SchState st = {0u, 0u, 0ull};
    uint32_t bsna = 0;
    bool interp = true, started = false, in_str = false, last_key = false;
    int32_t depth = 0;

    for (int64_t p0 = rbeg; p0 < rend; p0 += WAVE) {
        const int64_t left = rend - p0;   // >= 1 bytes of the span from p0 on
        const bool inr = lane < left;
        const uint32_t b = inr ? data[p0 + lane] : 0u;
        if (__ballot(b == '\\')) bsna |= SCH_BACKSLASH;
        if (__ballot(inr && (b >= 0x80u || b == 0u))) bsna |= SCH_NON_ASCII;
        if (!interp) continue;

        if (!started) {
            const uint64_t nonws = __ballot(inr && !sch_ws(b));
            if (!nonws) continue;
            const uint32_t fb = __shfl(b, __builtin_ctzll(nonws));
            if (fb != '{') {
                st.punt = SCH_NOT_OBJECT;
                interp = false;
                continue;
            }
            started = true;
        }

        const uint64_t quotes = __ballot(b == '"');
        uint64_t px = quotes;   // bit i: inside a string after lane i
        px ^= px << 1;
        px ^= px << 2;
        px ^= px << 4;
        px ^= px << 8;
        px ^= px << 16;
        px ^= px << 32;
        px ^= in_str ? ~0ull : 0ull;
        in_str = (px >> (WAVE - 1)) & 1ull;
        const uint64_t outside = ~px & ~quotes;
        const uint64_t opens = __ballot(b == '{' || b == '[') & outside;
        const uint64_t closes = __ballot(b == '}' || b == ']') & outside;
        const uint64_t upto = lanes_below(lane + 1);
        const int32_t dl = depth + __builtin_popcountll(opens & upto) - __builtin_popcountll(closes & upto);
        const uint64_t d1 = __ballot(dl == 1);
        const uint64_t key_s = (__ballot(b == '{') & opens & d1) | (__ballot(b == ',') & outside & d1);
        const uint64_t colon_s = __ballot(b == ':') & outside & d1;
        uint64_t keycand = quotes & px & d1;   // opening quotes at depth 1
        depth += __builtin_popcountll(opens) - __builtin_popcountll(closes);

        while (keycand) {
            const int t = __builtin_ctzll(keycand);
            keycand &= keycand - 1ull;
            const uint64_t kb = key_s & lanes_below(t), cb = colon_s & lanes_below(t);
            // the two are disjoint: the greater holds the nearest bit below t
            const bool is_key = (kb | cb) ? kb > cb : last_key;
            if (!is_key) continue;
            sch_key(data, (int32_t)p0 + t, rend, lane, lpow, lp10, pr, n_tp, tl.flags, enums, pool, st);
            if (st.punt) {
                interp = false;
                break;
            }
        }
        if (key_s | colon_s) last_key = key_s > colon_s;
    }

    uint32_t punt = bsna ? bsna : !started ? (uint32_t)SCH_NOT_OBJECT : st.punt;
    uint32_t fail = st.fail | ((tl.required & ~st.seen) ? (uint32_t)SCH_MISSING : 0u);
    if (lane == 0) {
        out_verdict[r] = punt ? SCH_PUNT : fail ? SCH_FAIL : SCH_PASS;
        out_fail[r] = punt ? 0 : (int32_t)fail;
        out_punt[r] = (int32_t)punt;
        out_seen[r] = punt ? 0ull : st.seen;
    }
}

extern "C" int forge_schema_check(
    const void* data, const void* beg, const void* end_, const void* tool_idx, int batch,
    const void* tools, int n_tools, const void* props, int n_props, const void* enums, int n_enums,
    const void* pool, int64_t pool_bytes,
    void* out_verdict, void* out_fail, void* out_punt, void* out_seen, void* stream)
{
    if (n_tools < 0 || n_tools > FORGE_SCHEMA_MAX_TOOLS || n_props < 0 || n_props > FORGE_SCHEMA_MAX_PROPS ||
        n_enums < 0 || n_enums > FORGE_SCHEMA_MAX_ENUMS || pool_bytes < 0 || pool_bytes > FORGE_SCHEMA_POOL_MAX)
        return FORGE_ERR_SCHEMA_CHECK;
    if (batch > 0 && (!out_verdict || !out_fail || !out_punt || !out_seen)) return FORGE_ERR_SCHEMA_CHECK;
    if (batch <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int in_lds = (n_tools <= FORGE_SCHEMA_LDS_TOOLS && n_props <= FORGE_SCHEMA_LDS_PROPS) ? 1 : 0;
    int grid = ceil_div(batch, ROW_WAVES);
    size_t lds = SCH_POW_BYTES + (in_lds ? FORGE_SCHEMA_LDS_TOOLS * FORGE_SCHEMA_TOOL_BYTES +
                                           (size_t)n_props * FORGE_SCHEMA_PROP_BYTES : 0);
    hipLaunchKernelGGL(schema_check_kernel, dim3(grid), dim3(ROW_WAVES * WAVE), lds, s,
                       (const uint8_t*)data, (const int32_t*)beg, (const int32_t*)end_, (const int32_t*)tool_idx, batch,
                       (const SchemaTool*)tools, n_tools, (const SchemaProp*)props, n_props, in_lds,
                       (const SchemaEnum*)enums, (const uint8_t*)pool,
                       (int32_t*)out_verdict, (int32_t*)out_fail, (int32_t*)out_punt, (uint64_t*)out_seen);
    return (int)hipGetLastError();
}
