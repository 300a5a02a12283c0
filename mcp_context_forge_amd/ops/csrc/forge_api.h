/* C ABI of libforge_hip.so: the one declaration of every exported forge_*
 * function. Every translation unit that defines one includes this header, so
 * the compiler checks definition against declaration; ops/hip.py mirrors it
 * in its ctypes table and tests/test_forge_abi.py checks that mirror.
 *
 * Plain C, no HIP includes, one declaration per statement. Device pointers
 * and hipStream_t cross the ABI as void*. */
#ifndef FORGE_API_H
#define FORGE_API_H

#include <stdint.h>

/* Epilogue activation codes (`act` of forge_gemm_bt* / forge_gemv_head). */
#define FORGE_ACT_NONE 0
#define FORGE_ACT_GELU 1    /* tanh approximation */
#define FORGE_ACT_SIGMOID 2

/* Argument errors of the kernel launchers; other non-zero returns are hipError_t. */
#define FORGE_ERR_SHAPE 9001      /* GEMM shape is not a multiple of the tile */
#define FORGE_ERR_ACT 9002        /* unknown activation code */
#define FORGE_ERR_GEMV_K 9003     /* gemv_head needs K % 512 == 0 */
#define FORGE_ERR_ROW_ALIGN 9004  /* row length must be a multiple of 8 bf16 */
#define FORGE_ERR_DECODE_SCAN 9005  /* decode_scan: bits, kw_max_len or keyword table size */
#define FORGE_ERR_SQL_SCAN 9006   /* sql_scan: n_kw, kw_max_len or keyword table size */
#define FORGE_ERR_RESCORE_ARGS 9007  /* rescore: row count, byte count, offsets or slot */
#define FORGE_ERR_RESCORE_BUSY 9008  /* rescore_submit: every slot is in use */

/* forge_scan* stage a bank's tables into LDS when they fit this many bytes;
 * ops/hip.py carries the same pair as SCAN_LDS_LIMIT / scan_table_bytes(). */
#define FORGE_SCAN_LDS_LIMIT (64 * 1024)
#define FORGE_SCAN_TABLE_BYTES(n_states, n_classes) \
    ((int64_t)(n_states) * (n_classes) * 2 + 256 + (int64_t)(n_states) * 4)

/* forge_decode_scan always stages its keyword tables into LDS: tables over
 * this many FORGE_SCAN_TABLE_BYTES, or a longest keyword over
 * FORGE_DECODE_SCAN_KW_MAX_LEN, are an argument error. ops/hip.py carries the
 * limit as DECODE_SCAN_TABLE_LIMIT. */
#define FORGE_DECODE_SCAN_TABLE_LIMIT (16 * 1024)
#define FORGE_DECODE_SCAN_KW_MAX_LEN 16

/* forge_sql_scan always stages its keyword tables into LDS too: tables over
 * this many FORGE_SCAN_TABLE_BYTES, a keyword count outside
 * FORGE_SQL_SCAN_MIN_KW..FORGE_SQL_SCAN_MAX_KW (five structural keywords plus
 * 1 to 24 blocked words) or a longest keyword outside
 * 2..FORGE_SQL_SCAN_KW_MAX_LEN are an argument error. ops/hip.py carries the
 * limit as SQL_SCAN_TABLE_LIMIT. */
#define FORGE_SQL_SCAN_TABLE_LIMIT (16 * 1024)
#define FORGE_SQL_SCAN_MIN_KW 6
#define FORGE_SQL_SCAN_MAX_KW 29
#define FORGE_SQL_SCAN_KW_MAX_LEN 16

typedef void (*forge_task_fn)(int index, void* ctx);

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device kernels (pointers are device memory; last argument is the stream) ---- */

int forge_scan(const void* data, const void* beg, const void* end_, int batch,
               const void* next, const void* klass, const void* accept,
               int n_states, int n_classes,
               void* out_mask, void* out_first_end, void* stream);

int forge_scan_multi(const void* data, const void* beg, const void* end_, int batch,
                     const void* descs_dev, int n_banks, int lds_bytes,
                     void* out_mask, void* stream);

/* One wave per request: entropy of the in-alphabet runs of at least min_len
 * bytes. sym is a 256-byte table, symbol 0..63 or 0xFF for a non-member.
 * out_h f32[batch], out_span i32[batch][2], out_runs / out_flags i32[batch]. */
int forge_token_entropy(const void* data, const void* beg, const void* end_, int batch,
                        const void* sym, int min_len,
                        void* out_h, void* out_span, void* out_runs, void* out_flags,
                        void* stream);

/* One wave per request: decode the in-alphabet runs of at least min_len bytes
 * (bits per symbol 4 or 6, MSB first), call a run text when
 * printable * 1000 >= min_printable_permille * dec_len, and match the keyword
 * DFA (next / klass / accept, longest keyword kw_max_len) over the decoded
 * bytes of text runs. out_counts i32[batch][3] (qualifying, text, text with a
 * keyword), out_kw u32[batch], out_span i32[batch][2], out_flags i32[batch]. */
int forge_decode_scan(const void* data, const void* beg, const void* end_, int batch,
                      const void* sym, int bits, int min_len, int min_printable_permille,
                      const void* next, const void* klass, const void* accept,
                      int n_states, int n_classes, int kw_max_len,
                      void* out_counts, void* out_kw, void* out_span, void* out_flags,
                      void* stream);

/* One wave per request: lex the span as SQL (strings, -- and block comments;
 * with dquote_boundary every '"' resets the lexer and closes the statement),
 * match whole words against the keyword DFA (keyword i has kw_len[i] bytes;
 * 0..4 are delete, from, update, set, where, the rest blocked words) and fold
 * per statement. out_counts i32[batch][4] (keyword statements, delete without
 * where, update without where, comments), out_blocked u32[batch] (bit i - 5),
 * out_first i32[batch][2] (absolute begin, length of the first finding or
 * -1, 0), out_flags i32[batch]. */
int forge_sql_scan(const void* data, const void* beg, const void* end_, int batch,
                   const void* next, const void* klass, const void* accept,
                   int n_states, int n_classes, const void* kw_len, int n_kw, int kw_max_len,
                   int dquote_boundary,
                   void* out_counts, void* out_blocked, void* out_first, void* out_flags,
                   void* stream);

int forge_featurize(const void* data, const void* beg, const void* end_, int batch, int dim,
                    void* out_bf16, void* out_f32, void* stream);

int forge_json_guard(const void* data, const void* beg, const void* end_, int batch,
                     int max_depth, int max_string,
                     void* out_status, void* out_depth, void* stream);

int forge_gemm_bt(const void* A, const void* BT, const void* bias, void* C,
                  int M, int N, int K, int act, int out_bf16, void* stream);

int forge_gemm_bt_v2(const void* A, const void* BT, const void* bias, void* C,
                     int M, int N, int K, int act, int out_bf16, void* stream);

/* 64x64 tiles for M <= ~1k (gemm_skinny.hip): M%64, N%64, K%64, else
 * FORGE_ERR_SHAPE with nothing launched. Bit-identical to the two above. */
int forge_gemm_bt_skinny(const void* A, const void* BT, const void* bias, void* C,
                         int M, int N, int K, int act, int out_bf16, void* stream);

int forge_gemv_head(const void* A, const void* WT, const void* bias, void* out,
                    int M, int C, int K, int act, void* stream);

int forge_rows_argmax_merge(const void* scores, int M, int Nc, int idx_base, const void* valid,
                            void* best_val, void* best_idx, void* stream);

int forge_rows_gather_scatter_bf16(const void* src, const void* src_rows, const void* dst_slots,
                                   void* dst, void* valid, int R, int D, void* stream);

int forge_verify_dot(const void* feats, const void* keys, const void* idx, void* out,
                     int M, int D, void* stream);

/* ---- native rescoring session (rescore.hip) ----
 * featurize + classifier + head over up to max_rows texts per submit, with
 * every buffer owned by the session: a submit allocates nothing and never
 * synchronises. w1t [hidden, dim] bf16, b1 f32[hidden], w2t [classes, hidden]
 * bf16 and b2 f32[classes] are device pointers the caller keeps alive.
 * max_rows, max_bytes (text bytes per submit) and n_slots <= 0 pick the
 * defaults 1024, 512 * max_rows and 4. One thread owns a session; only
 * forge_rescore_wait may run on another. Returns NULL on bad arguments or a
 * failed allocation. */
void* forge_rescore_new(const void* w1t, const void* b1, const void* w2t, const void* b2,
                        int dim, int hidden, int classes,
                        int max_rows, int64_t max_bytes, int n_slots);

/* blob / offs are HOST memory: offs int64[n + 1] (concat_with_offsets
 * layout), row i is blob[offs[i], offs[i + 1]). Returns the slot (>= 0) or a
 * negative FORGE_ERR_RESCORE_* / hipError_t; argument and busy errors return
 * before anything is launched. */
int forge_rescore_submit(void* ctx, const uint8_t* blob, const int64_t* offs, int n, void* stream);

/* 1 when the slot's scores are on the host, 0 while pending, negative on error. */
int forge_rescore_poll(void* ctx, int slot);

/* Blocks until the slot's scores are on the host: 1, or negative on error. */
int forge_rescore_wait(void* ctx, int slot);

/* Pinned host f32[max_rows][classes] of the slot; rows 0..n-1 are valid once
 * poll / wait returned 1 and until the slot is released. */
const float* forge_rescore_scores(void* ctx, int slot);

void forge_rescore_release(void* ctx, int slot);

void forge_rescore_free(void* ctx);

/* ---- host data plane (pointers are host memory) ---- */

void forge_parallel_for(int n, forge_task_fn fn, void* ctx);

int forge_parse_envelopes(const uint8_t* data, const int64_t* offsets, int n,
                          int32_t* kind, int32_t* id_beg, int32_t* id_end,
                          int32_t* name_beg, int32_t* name_end,
                          int32_t* args_beg, int32_t* args_end);

int64_t forge_upstream_call_batch(const uint8_t* data, const int32_t* args_beg,
                                  const int32_t* args_end, const int32_t* kinds, int n,
                                  const char* now_iso, uint8_t* out, int64_t out_cap,
                                  int64_t* res_beg, int64_t* res_end);

void* forge_store_new(int capacity);

void forge_store_put(void* store, int slot, const uint8_t* data, int64_t n);

void forge_store_put_batch(void* store, const int32_t* slots, int n,
                           const uint8_t* blob, const int64_t* beg, const int64_t* end);

int64_t forge_store_get(void* store, int slot, uint8_t* out, int64_t cap);

void forge_store_free(void* store);

void* forge_cache_new(double ttl);

void forge_cache_free(void* cache);

void* forge_toolmap_new(const uint8_t* blob, const int32_t* beg, const int32_t* end, int nt);

void forge_toolmap_free(void* map);

void forge_toolmap_resolve(void* map, const uint8_t* blob,
                           const int32_t* name_beg, const int32_t* name_end, int m,
                           int32_t* tool_idx_out);

int64_t forge_decide(
    const uint8_t* blob, const int32_t* id_beg, const int32_t* id_end,
    const int32_t* args_beg, const int32_t* args_end, const int32_t* tool_idx,
    const int32_t* name_beg, const int32_t* name_end,
    const uint32_t* deny_m, const uint32_t* harm_m, const uint32_t* pii_m,
    const uint32_t* regex_m, const uint32_t* norm_m, const uint32_t* schema_m,
    const uint8_t* mod_block, const int32_t* mod_cat, const float* mod_score,
    const uint8_t* hit, const int32_t* hit_slot, const uint64_t* user_hash, int m,
    const uint32_t* tool_flags, const uint32_t* tool_required_bits,
    const uint64_t* tool_typed_pairs,
    const int32_t* tname_beg, const int32_t* tname_end, const uint8_t* tname_blob,
    const int8_t* tool_native_kind, uint32_t nest_bits,
    const uint8_t* deny_words, const int32_t* deny_off, int n_deny,
    const uint8_t* harm_cats, const int32_t* harm_off, int n_harm,
    const uint8_t* mod_cats, const int32_t* mod_off, int n_mod,
    void* slot_store, void* exact_cache, double now,
    int32_t* state, int32_t* native_kind_out, int8_t* reason_out,
    uint8_t* arena, int64_t arena_cap, int64_t* resp_beg, int64_t* resp_end);

int64_t forge_finalize(
    const uint8_t* blob, const int32_t* id_beg, const int32_t* id_end,
    const int32_t* args_beg, const int32_t* args_end, const int32_t* tool_idx,
    const uint64_t* user_hash, int m, const int32_t* rows, int n_rows,
    const uint8_t* res_blob, const int64_t* res_beg, const int64_t* res_end,
    const uint8_t* needs_host,
    const int32_t* tname_beg, const int32_t* tname_end, const uint8_t* tname_blob,
    const uint32_t* tool_flags,
    void* exact_cache, double now, double exact_ttl,
    uint8_t* arena, int64_t arena_cap, int64_t* resp_beg, int64_t* resp_end,
    uint8_t* is_error_out, uint8_t* cacheable_out);

int64_t forge_rewrite_rows(
    const uint8_t* blob, const int32_t* args_beg, const int32_t* args_end, int n,
    const uint8_t* do_flags, const uint32_t* pii_want,
    uint32_t pii_active_mask, int pii_mode, int norm_collapse, int norm_strip,
    const uint8_t* deny_blob, const int32_t* deny_off, int n_deny, int deny_ci,
    int32_t* status, uint32_t* found_bits, int32_t* deny_hit,
    uint8_t* arena, int64_t arena_cap,
    int64_t* out_beg, int64_t* out_end, int64_t* scan_beg, int64_t* scan_end,
    const uint8_t* harm_blob, const int32_t* harm_off, int n_harm, int32_t* harm_out,
    const uint8_t* sk_blob, const int32_t* sk_beg, const int32_t* sk_end,
    const int8_t* sk_type, const uint8_t* sk_req,
    const int32_t* sk_lo, const int32_t* sk_hi, uint8_t* schema_out);

int64_t forge_post_rows(
    const uint8_t* blob, const int64_t* res_beg, const int64_t* res_end, int n,
    const uint8_t* do_flags, uint32_t pii_active_mask, int pii_mode,
    const uint8_t* harm_blob, const int32_t* harm_off, int n_harm,
    int64_t toon_min_size, double toon_min_savings,
    int32_t* status, uint32_t* found_bits, int32_t* harm_hit, uint8_t* is_err,
    uint8_t* arena, int64_t arena_cap, int64_t* out_beg, int64_t* out_end);

#ifdef __cplusplus
}
#endif

#endif /* FORGE_API_H */
