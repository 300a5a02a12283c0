// Per-request SQL lexer, whole-word keyword match and per-statement fold: the
// kernel half of sql_sanitizer.
//
// "A blocked keyword in code, not inside a string or a comment" and "DELETE
// without WHERE in one statement" need lexer state carried along the request
// and a fold per statement, which the search-semantics DFA banks of scan.hip
// cannot express. Semantics are identical to ops/sql.py sql_scan_reference —
// the CPU oracle in tests and the code the plugin itself runs.
//
// The lexer has the states CODE, SQUOTE, DQUOTE, LINE (-- … \n) and BLOCK
// (/* … */). In CODE a maximal run of [A-Za-z0-9_] is a word; a word of
// length L matches keyword i when the keyword DFA, walked from state 0 over
// the word, accepts i and kw_len[i] == L. Keywords 0..4 are delete, from,
// update, set, where; the blocked words follow from bit 5. A statement closes
// at ';' in CODE, at the span end and — with dquote_boundary — at every '"',
// which then also resets the lexer to CODE from any state.
//
// Parallelization: one wavefront per request, as entropy.hip and exfil.hip.
// Each step loads 64 bytes (one per lane) plus up to 32 bytes of lookahead,
// and takes ballots for the bytes that can move the lexer. The lexer is
// sequential but sparse: only the events that matter in the current state are
// walked with ctz, building a 64-bit mask of CODE lanes and a mask of
// statement terminators. A two-byte token consumes its second byte; when it
// sits in lane 63 a "skip lane 0" bit is carried. Word characters never move
// the lexer, so a word's first byte decides for the whole word: a word start
// is a word character in CODE whose predecessor is none, and that lane walks
// the DFA over at most kw_max_len + 1 bytes of a per-wave LDS window (chunk +
// lookahead, zero past the span end). A word that straddles the chunk edge is
// owned by its start lane, so no word state is carried. The statement fold
// takes one ballot per structural keyword and walks the terminator mask,
// carrying (mask, first delete, first update) of the open statement.
//
// The carries are the lexer state, the skip bit, "previous byte was a word
// character" and the open statement. All control flow derives from ballots
// and kernel arguments, so every branch is wave-uniform; per-lane conditions
// are selects.

#include "common.h"

#define SQL_WAVES 4       // waves (= requests) per block
#define SQL_LOOKAHEAD 32  // bytes after the chunk in the window (>= FORGE_SQL_SCAN_KW_MAX_LEN + 1)
#define SQL_WIN (WAVE + SQL_LOOKAHEAD)
#define SQL_LENMASKS 32   // keyword masks by word length, 0..31

static_assert(SQL_LOOKAHEAD >= FORGE_SQL_SCAN_KW_MAX_LEN + 1 && SQL_LENMASKS > FORGE_SQL_SCAN_KW_MAX_LEN + 1,
              "a word start in lane 63 walks kw_max_len + 1 bytes");

enum { SQL_CODE = 0, SQL_SQUOTE, SQL_DQUOTE, SQL_LINE, SQL_BLOCK };

// lanes [0, n) as a mask; n may be 64 or 65
__device__ __forceinline__ uint64_t sql_below(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }

__device__ __forceinline__ bool sql_word_char(uint32_t b) {
    const uint32_t l = b | 0x20u;
    return (b >= '0' && b <= '9') || (l >= 'a' && l <= 'z') || b == '_';
}

__global__ __launch_bounds__(SQL_WAVES * WAVE) void sql_scan_kernel(
    const uint8_t* __restrict__ data,    // packed bytes
    const int32_t* __restrict__ beg,
    const int32_t* __restrict__ end_,
    int batch,
    const uint16_t* __restrict__ next,   // keyword DFA [S, C]
    const uint8_t* __restrict__ klass,   // [256]
    const uint32_t* __restrict__ accept, // [S]
    int n_states, int n_classes,
    const int32_t* __restrict__ kw_len,  // [n_kw]
    int n_kw, int kw_max_len, int dquote_boundary,
    int32_t* __restrict__ out_counts,    // [B, 4] keyword statements, delete / update without where, comments
    uint32_t* __restrict__ out_blocked,  // [B] bit i - 5 for blocked keyword i
    int32_t* __restrict__ out_first,     // [B, 2] absolute begin, length of the finding with the smallest begin; (-1, 0)
    int32_t* __restrict__ out_flags)     // [B] bit 0: span holds a backslash or a byte >= 0x80
{
    // lenmask u32[32] | accept u32[S] | next u16[S*C] | klass u8[256] | per wave: window
    extern __shared__ __align__(16) uint8_t lds_raw[];
    uint32_t* llen = (uint32_t*)lds_raw;
    uint32_t* laccept = llen + SQL_LENMASKS;
    uint16_t* lnext = (uint16_t*)(laccept + n_states);
    uint8_t* lklass = (uint8_t*)(lnext + (size_t)n_states * n_classes);
    uint8_t* win = lklass + 256 + (threadIdx.x / WAVE) * SQL_WIN;
    for (int i = threadIdx.x; i < n_states; i += blockDim.x) laccept[i] = accept[i];
    for (int i = threadIdx.x; i < n_states * n_classes; i += blockDim.x) lnext[i] = next[i];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) lklass[i] = klass[i];
    if (threadIdx.x < SQL_LENMASKS) {
        // the keywords of exactly this length
        uint32_t mk = 0;
        for (int i = 0; i < n_kw; ++i) mk |= kw_len[i] == (int32_t)threadIdx.x ? (1u << i) : 0u;
        llen[threadIdx.x] = mk;
    }
    // every wave of the block reaches this barrier before any wave leaves
    __syncthreads();

    const int lane = threadIdx.x & (WAVE - 1);
    const int r = blockIdx.x * SQL_WAVES + (threadIdx.x / WAVE);
    if (r >= batch) return;  // wave-uniform
    const int32_t rbeg = beg[r], rend = end_[r];

    // lexer carries
    int state = SQL_CODE;
    int skip0 = 0;            // lane 0 is the second byte of a token begun in the previous chunk
    uint64_t prev_wc = 0;     // bit 0: the previous chunk's last byte was a word character
    // open statement: structural bits 0..4, bit 5 for any blocked word
    uint32_t st_mask = 0;
    int32_t st_del = -1, st_upd = -1;
    int32_t n_stmt = 0, n_dww = 0, n_uww = 0, n_com = 0, flags = 0, first_beg = -1, first_len = 0;
    uint32_t blocked = 0;

    auto finding = [&](int32_t b, int32_t l) {
        if (first_beg < 0 || b < first_beg) {
            first_beg = b;
            first_len = l;
        }
    };

    auto close_stmt = [&]() {
        if (st_mask) {
            ++n_stmt;
            if ((st_mask & 3u) == 3u && !(st_mask & 16u)) {
                ++n_dww;
                finding(st_del, 6);
            }
            if ((st_mask & 12u) == 12u && !(st_mask & 16u)) {
                ++n_uww;
                finding(st_upd, 6);
            }
        }
        st_mask = 0;
        st_del = -1;
        st_upd = -1;
    };

    for (int32_t p = rbeg; p < rend; p += WAVE) {
        const int32_t left = rend - p;   // >= 1 bytes of the span from p on
        const uint8_t* __restrict__ chunk = data + p;
        const uint32_t b = lane < left ? chunk[lane] : 0u;
        const uint32_t la = (lane < SQL_LOOKAHEAD && lane < left - WAVE) ? chunk[WAVE + lane] : 0u;
        // cross-lane reads stand in statements of their own: inside a conditional
        // operand only the selected lanes would take part in the exchange
        const uint32_t up = __shfl_down(b, 1);
        const uint32_t la0 = __builtin_amdgcn_readfirstlane(la);
        const uint32_t nb = lane == WAVE - 1 ? la0 : up;   // the byte after this lane's
        if (__ballot(b == '\\' || b >= 0x80u)) flags = 1;
        const uint64_t q1 = __ballot(b == '\'');
        const uint64_t q2 = __ballot(b == '"');
        const uint64_t dd = __ballot(b == '-' && nb == '-');
        const uint64_t bo = __ballot(b == '/' && nb == '*');
        const uint64_t bc = __ballot(b == '*' && nb == '/');
        const uint64_t nl = __ballot(b == '\n');
        const uint64_t semi = __ballot(b == ';');
        const uint64_t wc = __ballot(sql_word_char(b));
        const uint64_t bq = dquote_boundary ? q2 : 0ull;

        // lexer: walk the events that matter in the current state
        uint64_t code = 0, term = 0;
        int pos = skip0;
        while (pos < WAVE) {
            uint64_t ev;
            switch (state) {
                case SQL_CODE: ev = q1 | q2 | dd | bo | semi; break;
                case SQL_SQUOTE: ev = q1 | bq; break;
                case SQL_DQUOTE: ev = q2; break;
                case SQL_LINE: ev = nl | bq; break;
                default: ev = bc | bq; break;
            }
            ev &= ~sql_below(pos);
            if (!ev) {
                if (state == SQL_CODE) code |= ~sql_below(pos);
                break;
            }
            const int t = __builtin_ctzll(ev);
            const uint64_t bit = 1ull << t;
            if (state == SQL_CODE) code |= sql_below(t) & ~sql_below(pos);
            pos = t + 1;
            if (bit & bq) {                 // field boundary, in any state
                state = SQL_CODE;
                term |= bit;
            } else if (state == SQL_CODE) {
                if (bit & q1) {
                    state = SQL_SQUOTE;
                } else if (bit & q2) {
                    state = SQL_DQUOTE;
                } else if (bit & dd) {
                    state = SQL_LINE;
                    ++n_com;
                    pos = t + 2;
                } else if (bit & bo) {
                    state = SQL_BLOCK;
                    ++n_com;
                    pos = t + 2;
                } else {
                    term |= bit;            // ;
                }
            } else {
                if (state == SQL_BLOCK) pos = t + 2;
                state = SQL_CODE;
            }
        }
        skip0 = pos == WAVE + 1 ? 1 : 0;

        // whole-word match, by the lane of the word's first byte
        const uint64_t ws = wc & code & ~((wc << 1) | prev_wc);
        prev_wc = wc >> (WAVE - 1);
        uint32_t m = 0;
        int32_t wlen = 0;
        if (ws) {
            win[lane] = (uint8_t)b;
            if (lane < SQL_LOOKAHEAD) win[WAVE + lane] = (uint8_t)la;
            // the window is written and read by different lanes of this wave
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            bool alive = (ws >> lane) & 1ull;
            uint32_t s = 0;
            for (int i = 0; i <= kw_max_len; ++i) {
                const uint32_t c = win[lane + i];
                alive = alive && sql_word_char(c);
                const uint32_t ns = lnext[s * n_classes + lklass[c]];
                s = alive ? ns : s;
                wlen += alive ? 1 : 0;
            }
            // wlen == kw_max_len + 1 stands for every longer word: no keyword has that length
            m = laccept[s] & llen[wlen];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }

        // statement fold
        const uint64_t kany = __ballot(m != 0u);
        if (kany) {
            const uint64_t kdel = __ballot((m & 1u) != 0u), kfrom = __ballot((m & 2u) != 0u);
            const uint64_t kupd = __ballot((m & 4u) != 0u), kset = __ballot((m & 8u) != 0u);
            const uint64_t kwhere = __ballot((m & 16u) != 0u), kblk = __ballot((m >> 5) != 0u);
            if (kblk) {
                uint32_t mb = m >> 5;
                #pragma unroll
                for (int off = WAVE / 2; off > 0; off >>= 1) mb |= __shfl_xor(mb, off);
                blocked |= __builtin_amdgcn_readfirstlane(mb);
                const int t = __builtin_ctzll(kblk);
                finding(p + t, __shfl(wlen, t));
            }
            int cur = 0;
            while (true) {
                const uint64_t tt = term & ~sql_below(cur);
                const int e = tt ? __builtin_ctzll(tt) : WAVE;
                const uint64_t seg = sql_below(e) & ~sql_below(cur);
                if (kany & seg) {
                    if (st_del < 0 && (kdel & seg)) st_del = p + __builtin_ctzll(kdel & seg);
                    if (st_upd < 0 && (kupd & seg)) st_upd = p + __builtin_ctzll(kupd & seg);
                    st_mask |= ((kdel & seg) ? 1u : 0u) | ((kfrom & seg) ? 2u : 0u) | ((kupd & seg) ? 4u : 0u) |
                               ((kset & seg) ? 8u : 0u) | ((kwhere & seg) ? 16u : 0u) | ((kblk & seg) ? 32u : 0u);
                }
                if (e == WAVE) break;
                close_stmt();
                cur = e + 1;
            }
        } else if (term) {
            close_stmt();   // every further terminator of this chunk closes an empty statement
        }
    }
    close_stmt();   // the span end closes the open statement

    if (lane == 0) {
        out_counts[4 * r] = n_stmt;
        out_counts[4 * r + 1] = n_dww;
        out_counts[4 * r + 2] = n_uww;
        out_counts[4 * r + 3] = n_com;
        out_blocked[r] = blocked;
        out_first[2 * r] = first_beg;
        out_first[2 * r + 1] = first_len;
        out_flags[r] = flags;
    }
}

extern "C" int forge_sql_scan(
    const void* data, const void* beg, const void* end_, int batch,
    const void* next, const void* klass, const void* accept,
    int n_states, int n_classes, const void* kw_len, int n_kw, int kw_max_len,
    int dquote_boundary,
    void* out_counts, void* out_blocked, void* out_first, void* out_flags, void* stream)
{
    if (n_kw < FORGE_SQL_SCAN_MIN_KW || n_kw > FORGE_SQL_SCAN_MAX_KW) return FORGE_ERR_SQL_SCAN;
    if (kw_max_len < 2 || kw_max_len > FORGE_SQL_SCAN_KW_MAX_LEN) return FORGE_ERR_SQL_SCAN;
    if (n_states < 1 || n_classes < 1 ||
        FORGE_SCAN_TABLE_BYTES(n_states, n_classes) > FORGE_SQL_SCAN_TABLE_LIMIT)
        return FORGE_ERR_SQL_SCAN;
    if (batch <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int grid = ceil_div(batch, SQL_WAVES);
    size_t lds = (size_t)FORGE_SCAN_TABLE_BYTES(n_states, n_classes) + SQL_LENMASKS * 4 + SQL_WAVES * SQL_WIN;
    hipLaunchKernelGGL(sql_scan_kernel, dim3(grid), dim3(SQL_WAVES * WAVE), lds, s,
                       (const uint8_t*)data, (const int32_t*)beg, (const int32_t*)end_, batch,
                       (const uint16_t*)next, (const uint8_t*)klass, (const uint32_t*)accept,
                       n_states, n_classes, (const int32_t*)kw_len, n_kw, kw_max_len, dquote_boundary ? 1 : 0,
                       (int32_t*)out_counts, (uint32_t*)out_blocked, (int32_t*)out_first, (int32_t*)out_flags);
    return (int)hipGetLastError();
}
