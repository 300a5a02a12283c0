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
#define FORGE_ERR_URL_SCAN 9009   /* url_scan: slot count, pool size or report_mask */
#define FORGE_ERR_ACCOUNT_SCAN 9010   /* account_scan: report_mask */
#define FORGE_ERR_UNICODE_SCAN 9011   /* unicode_scan: n_ranges or report_mask */
#define FORGE_ERR_JSON_UNESCAPE 9012  /* json_unescape: a null output with batch > 0 */
#define FORGE_ERR_SEMCACHE_TOPK 9013  /* sketch_topk / verify_topk: k, S, B, D, splits or a null output */
#define FORGE_ERR_SCHEMA_CHECK 9014   /* schema_check: a table count or a null output with batch > 0 */

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

/* forge_url_scan probes a domain table of up to FORGE_URL_SCAN_LDS_SLOTS
 * slots in LDS (staged once per block) and a larger one in global memory. A
 * slot count that is no power of two or outside
 * FORGE_URL_SCAN_MIN_SLOTS..FORGE_URL_SCAN_MAX_SLOTS, a pool over
 * FORGE_URL_SCAN_POOL_MAX bytes or a report_mask with bits outside
 * FORGE_URL_SCAN_ALL_BITS are an argument error. An authority is analysed up
 * to FORGE_URL_SCAN_AUTH_MAX bytes. ops/hip.py carries the first as
 * URL_SCAN_LDS_SLOTS; ops/url.py has them all. */
#define FORGE_URL_SCAN_LDS_SLOTS 1024
#define FORGE_URL_SCAN_MIN_SLOTS 2
#define FORGE_URL_SCAN_MAX_SLOTS (1 << 20)
#define FORGE_URL_SCAN_POOL_MAX ((int64_t)1 << 31)
#define FORGE_URL_SCAN_ALL_BITS 1023
#define FORGE_URL_SCAN_AUTH_MAX 256

/* forge_account_scan reads a table of FORGE_ACCOUNT_SCAN_TABLE_BYTES country
 * lengths, indexed 26 * (c0 - 'A') + (c1 - 'A'); an entry outside
 * FORGE_ACCOUNT_SCAN_MIN_LEN..FORGE_ACCOUNT_SCAN_MAX_LEN is an unknown
 * country. A report_mask with bits outside FORGE_ACCOUNT_SCAN_ALL_KINDS (1
 * card, 2 IBAN) is an argument error. ops/account.py has them all. */
#define FORGE_ACCOUNT_SCAN_TABLE_BYTES 676
#define FORGE_ACCOUNT_SCAN_MIN_LEN 15
#define FORGE_ACCOUNT_SCAN_MAX_LEN 34
#define FORGE_ACCOUNT_SCAN_ALL_KINDS 3

/* forge_unicode_scan searches a class table of up to
 * FORGE_UNICODE_SCAN_MAX_RANGES ranges of FORGE_UNICODE_SCAN_RANGE_BYTES bytes
 * (u32 lo, hi, kinds, script; sorted, disjoint, above ASCII), staged into LDS
 * once per block. A range count outside 0..FORGE_UNICODE_SCAN_MAX_RANGES or a
 * report_mask with bits outside FORGE_UNICODE_SCAN_ALL_KINDS (the
 * FORGE_UNICODE_SCAN_KINDS kind bits: bidi, invisible, tag, variation, joiner,
 * private, invalid, mixed script) is an argument error. ops/unicode.py has
 * them all. */
#define FORGE_UNICODE_SCAN_MAX_RANGES 256
#define FORGE_UNICODE_SCAN_RANGE_BYTES 16
#define FORGE_UNICODE_SCAN_KINDS 8
#define FORGE_UNICODE_SCAN_ALL_KINDS 255

/* forge_schema_check walks tables of FORGE_SCHEMA_TOOL_BYTES, _PROP_BYTES and
 * _ENUM_BYTES records (ops/schema.py lays them out and validates them before
 * upload). A tool has at most FORGE_SCHEMA_MAX_TOOL_PROPS properties, one per
 * lane. Tables of up to FORGE_SCHEMA_LDS_TOOLS tools and FORGE_SCHEMA_LDS_PROPS
 * properties are staged into LDS once per block, larger ones are read from
 * global memory. Counts outside 0..FORGE_SCHEMA_MAX_TOOLS / _PROPS / _ENUMS or a
 * pool over FORGE_SCHEMA_POOL_MAX bytes are an argument error. ops/schema.py
 * has them all. */
#define FORGE_SCHEMA_TOOL_BYTES 24
#define FORGE_SCHEMA_PROP_BYTES 40
#define FORGE_SCHEMA_ENUM_BYTES 16
#define FORGE_SCHEMA_MAX_TOOL_PROPS 64
#define FORGE_SCHEMA_LDS_TOOLS 64
#define FORGE_SCHEMA_LDS_PROPS 256
#define FORGE_SCHEMA_MAX_TOOLS 4096
#define FORGE_SCHEMA_MAX_PROPS (1 << 18)
#define FORGE_SCHEMA_MAX_ENUMS (1 << 20)
#define FORGE_SCHEMA_POOL_MAX ((int64_t)1 << 24)

/* forge_sketch_topk keeps 1..FORGE_SKETCH_TOPK_MAX_K candidates per row. Its
 * grid is (B / 64) x splits; a split sweeps at most FORGE_SKETCH_TOPK_MAX_TILES
 * tiles of 64 slots and there are at most FORGE_SKETCH_TOPK_MAX_SPLITS, so one
 * launch covers 64 * 512 * 64 slots. With splits == 0 the launcher takes the
 * fewest splits that give FORGE_SKETCH_TOPK_TARGET_BLOCKS workgroups (two per
 * CU of a 256-CU part), at most one per slot tile and at most the cap. A
 * workgroup uses FORGE_SKETCH_TOPK_LDS_BYTES(S) bytes of LDS: the query tile
 * (128 * S) plus a 3-chunk key ring, one score tile, the slot metadata ring,
 * the row identities and the live-tile list (47744): 80512 at S = 256, two
 * workgroups per 160 KiB CU; 113280 at the cap S = 512. forge_verify_topk
 * holds a feature row of up to FORGE_VERIFY_TOPK_MAX_D bf16 in registers.
 * ops/hip.py carries MAX_K and MAX_SPLITS as SKETCH_TOPK_MAX_K / _MAX_SPLITS. */
#define FORGE_SKETCH_TOPK_MAX_K 8
#define FORGE_SKETCH_TOPK_MAX_SPLITS 64
#define FORGE_SKETCH_TOPK_MAX_TILES 512
#define FORGE_SKETCH_TOPK_TARGET_BLOCKS 512
#define FORGE_SKETCH_TOPK_LDS_BYTES(S) ((S) * 128 + 47744)
#define FORGE_VERIFY_TOPK_MAX_D 8192

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

/* One wave per request: every "://" with a scheme before it is a URL; delimit
 * its authority and host (userinfo, port, trailing dots), classify it (bits
 * 0..9: blocked, http, other scheme, numeric, bracket, userinfo, punycode,
 * non-ascii, overlong, empty host) and look every label-start suffix of the
 * host up in the domain table: slots u32[n_slots][4] (key, tag 1 blocked / 2
 * allowed / 0 empty, pool offset, length), pool the domain bytes, powers
 * u32[2][256]; an allowed suffix beats a blocked one. out_counts
 * i32[batch][4] (urls, allowed, blocked-domain, reported: bits & report_mask),
 * out_mask i32[batch], out_first i32[batch][2] (absolute begin, length of the
 * first reported URL or -1, 0), out_flags i32[batch]. */
int forge_url_scan(const void* data, const void* beg, const void* end_, int batch,
                   const void* slots, int n_slots, const void* pool, int64_t pool_bytes,
                   const void* powers, int report_mask,
                   void* out_counts, void* out_mask, void* out_first, void* out_flags,
                   void* stream);

/* One wave per request: payment cards (runs of 13..19 digits with single ' '
 * or '-' separators, first digit not 0, no [A-Za-z_.] before and no [A-Za-z_]
 * after, valid by Luhn) and IBANs (two letters, two digits, the length
 * iban_len u8[676] gives for the country, single spaces allowed, valid when
 * the rotated base-36 number is 1 mod 97). out_counts i32[batch][4] (card
 * candidates, valid cards, IBAN candidates, valid IBANs), out_kinds i32[batch]
 * (bit 0 a valid card, bit 1 a valid IBAN), out_first i32[batch][2] (absolute
 * begin, length of the first valid finding of a kind in report_mask, or -1, 0),
 * out_flags i32[batch]. */
int forge_account_scan(const void* data, const void* beg, const void* end_, int batch,
                       const void* iban_len, int report_mask,
                       void* out_counts, void* out_kinds, void* out_first, void* out_flags,
                       void* stream);

/* One wave per request: UTF-8 decoded strictly (an ill-formed byte is one
 * INVALID event), every multi-byte code point classified against table
 * (n_ranges ranges), words of ASCII [A-Za-z0-9_] and script-bearing code points
 * judged mixed when they hold a Latin and a Greek or Cyrillic letter.
 * out_counts i32[batch][8] (code points per kind bit, INVALID events, mixed
 * words), out_kinds i32[batch] (the bits with a non-zero count), out_first
 * i32[batch][2] (absolute begin, byte length of the first finding of a kind in
 * report_mask, or -1, 0), out_flags i32[batch] (bit 0 a backslash, bit 1 a
 * byte >= 0x80). */
int forge_unicode_scan(const void* data, const void* beg, const void* end_, int batch,
                       const void* table, int n_ranges, int report_mask,
                       void* out_counts, void* out_kinds, void* out_first, void* out_flags,
                       void* stream);

/* One wave per request: walk the JSON structure of data[beg[r], end_[r])
 * against the compiled schema of tool tool_idx[r] i32[batch] (schema.hip;
 * ops/schema.py schema_check_reference is the definition). tools, props,
 * enums, pool: the tables of ops/schema.py compile_schemas in device memory.
 * Writes every element of out_verdict i32[batch] (0 PASS, 1 FAIL, 2 PUNT),
 * out_fail i32[batch] (bit 0 missing required, 1 type, 2 enum, 3 bound,
 * 4 length, 5 additional), out_punt i32[batch] (bit 0 backslash, 1 non-ASCII,
 * 2 not an object, 3 long, 4 duplicate key, 5 number form, 6 no table) and
 * out_seen u64[batch] (the tool's properties met); with a punt, fail and seen
 * are 0. PASS implies that utils/jsonschema.validate accepts the decoded
 * span. An empty batch launches nothing. */
int forge_schema_check(const void* data, const void* beg, const void* end_, const void* tool_idx, int batch,
                       const void* tools, int n_tools, const void* props, int n_props,
                       const void* enums, int n_enums, const void* pool, int64_t pool_bytes,
                       void* out_verdict, void* out_fail, void* out_punt, void* out_seen,
                       void* stream);

/* One wave per request: the JSON string escapes of data[beg, end) decoded into
 * out (as large as data), request r's bytes at out[beg[r], out_end[r]); the
 * output is never longer than the input and bytes of out outside those ranges
 * are unspecified. Short escapes give their byte, \uXXXX its UTF-8, a surrogate
 * pair one 4-byte sequence, a lone surrogate EF BF BD, and a malformed
 * backslash is copied. out_end i32[batch], out_flags i32[batch] (bit 0 an
 * escape was decoded, 1 a decoded quote, 2 a decoded or malformed backslash,
 * 3 a malformed escape, 4 a lone surrogate, 5 a decoded U+0000, 6 a decoded
 * code point >= 0x80); every element is written. ops/unescape.py has them
 * all. */
int forge_json_unescape(const void* data, const void* beg, const void* end_, int batch,
                        void* out, void* out_end, void* out_flags, void* stream);

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

/* The fused sketch sweep of the semantic cache (semcache.hip): for each of the
 * B rows of q_sk [B, S] bf16, the k best eligible slots of keys_sk in the
 * order (score descending, slot ascending), padded with (-1e30, -1). Slot c
 * is eligible for row r when c < active, valid[c] != 0, ident[c] ==
 * q_ident[r] (i64) and stamp[c] >= min_stamp (u32). Scores have the bits of
 * forge_gemm_bt and never reach global memory. keys_sk, ident, stamp and valid
 * hold at least active rounded up to 64 slots; valid is 4-byte aligned. partial_val f32 / partial_idx
 * i32 [B, splits, k] are scratch (FORGE_SKETCH_TOPK_MAX_SPLITS covers
 * splits == 0); out_val f32 / out_idx i32 [B, k]; every element of out_* is
 * written and does not depend on splits. active == 0 launches only the merge
 * kernel, which writes the padding; B == 0 launches nothing. k outside
 * 1..FORGE_SKETCH_TOPK_MAX_K, S no multiple of 64 in 64..512, B no multiple
 * of 64, active < 0, splits outside 0..FORGE_SKETCH_TOPK_MAX_SPLITS or too few
 * for active (FORGE_SKETCH_TOPK_MAX_TILES per split), a null out_* or, with
 * active > 0, a null partial_* return FORGE_ERR_SEMCACHE_TOPK with nothing
 * launched. */
int forge_sketch_topk(const void* q_sk, const void* keys_sk, const void* ident, const void* stamp,
                      const void* valid, const void* q_ident, uint32_t min_stamp, int active,
                      int B, int S, int k, int splits,
                      void* partial_val, void* partial_idx, void* out_val, void* out_idx,
                      void* stream);

/* One wave per row: the exact bf16 dot (the bits of forge_verify_dot) of
 * feats[r] with keys[cand[r, j]] for every cand[r, j] >= 0, j < k; best_val
 * f32[M] the greatest, best_idx i32[M] its slot, the first listed on a tie,
 * (-1e30, -1) for a row without a candidate. Every element is written.
 * D % 8 returns FORGE_ERR_ROW_ALIGN; k outside 1..FORGE_SKETCH_TOPK_MAX_K or
 * D outside 8..FORGE_VERIFY_TOPK_MAX_D FORGE_ERR_SEMCACHE_TOPK. */
int forge_verify_topk(const void* feats, const void* keys, const void* cand, int k, int M, int D,
                      void* best_val, void* best_idx, void* stream);

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
